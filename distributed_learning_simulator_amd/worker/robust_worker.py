"""Attack injection for the robust aggregation methods (`fed_trimmed_mean`, `fed_median`).

`ByzantineWorker` is an AggregationWorker whose clients with id < `algorithm_kwargs.byzantine_number`
(default 0: nobody) are Byzantine: after the honest upload rows are formed, their rows are
overwritten in place according to `algorithm_kwargs.byzantine_attack`:

* `sign_flip` (default): row ← −`byzantine_scale` · row (scale default 10);
* `nan`: every parameter NaN;
* `inf`: +inf at even flat indices, −inf at odd ones;
* `gauss`: `byzantine_scale` · N(0, 1), hash-keyed by client id and round (`fl.row_seeds`), so the
  noise does not depend on which rank or wave hosts the client.

Inter-tensor padding stays +0. Plain torch ops: an attack is not a hot path.
"""

from __future__ import annotations

import math

import torch

from ..message import CohortMessage
from ..ops import fl
from .aggregation_worker import AggregationWorker

ATTACKS = ("sign_flip", "nan", "inf", "gauss")


class ByzantineWorker(AggregationWorker):
    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        kw = config.algorithm_kwargs
        self.byzantine_number = int(kw.get("byzantine_number", 0) or 0)
        self.byzantine_attack = str(kw.get("byzantine_attack", "sign_flip"))
        self.byzantine_scale = float(kw.get("byzantine_scale", 10.0))
        if self.byzantine_attack not in ATTACKS:
            raise ValueError(f"byzantine_attack must be one of {ATTACKS}, got {self.byzantine_attack!r}")

    def _gauss_rows(self, clients: list[int], P: int, device) -> torch.Tensor:
        base = (self.config.seed * 2_750_159 + self._round_num * 15_485_863) & 0x7FFFFFFF
        u1 = fl.uniform_rows(fl.row_seeds(base, clients), P, device)
        u2 = fl.uniform_rows(fl.row_seeds(base ^ 0x5BD1E995, clients), P, device)
        return torch.sqrt(-2.0 * torch.log1p(-u1)) * torch.cos((2.0 * math.pi) * u2)  # Box–Muller

    def _get_sent_data(self, wave, theta_g, stats) -> CohortMessage:
        msg = super()._get_sent_data(wave, theta_g, stats)
        bad = [i for i, c in enumerate(wave) if c < self.byzantine_number]
        if not bad:
            return msg
        rows = msg.data
        P, dev = rows.shape[1], rows.device
        sel = torch.tensor(bad, device=dev)
        attack = self.byzantine_attack
        if attack == "sign_flip":
            evil = rows[sel] * (-self.byzantine_scale)
        elif attack == "nan":
            evil = torch.full((len(bad), P), float("nan"), dtype=rows.dtype, device=dev)
        elif attack == "inf":
            signs = torch.where(torch.arange(P, device=dev) % 2 == 0, float("inf"), float("-inf"))
            evil = signs.to(rows.dtype).expand(len(bad), P)
        else:
            evil = self._gauss_rows([wave[i] for i in bad], P, dev).to(rows.dtype) * self.byzantine_scale
        valid = self.trainer.layout.valid_mask(dev)
        rows[sel] = torch.where(valid, evil, torch.zeros((), dtype=rows.dtype, device=dev))
        return msg
