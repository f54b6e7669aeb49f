"""Krum and Multi-Krum (Blanchard et al. 2017, "Machine learning with adversaries: Byzantine
tolerant gradient descent"): whole uploads are chosen by their distance to the other uploads. Not
in the reference. Unlike the coordinate-wise statistics of `robust_algorithm.py`, Krum returns a
model that some client actually trained.

The round's rows [n, P] are stored and all-gathered as for the trimmed mean (`TrimmedMeanAlgorithm`),
with the client ids travelling along. `ops.fl.pairwise_sq_dists` (csrc/krum.hip; oracle ops/ref.py)
gives the n x n squared distances in fp64 with a fixed summation order, so every rank, and the CPU
oracle, hold the same bits; `ops.fl.krum_select` scores each row on the host (the sum of its
n − f − 2 smallest distances to other rows) and keeps the m rows with the smallest (score, client
id). f = `algorithm_kwargs.krum_f`, default `byzantine_number`.

* `fed_krum` (m = 1): θ_{t+1} = θ_t + row for delta uploads, the row itself for parameter uploads —
  one client's upload, verbatim.
* `fed_multi_krum` (m = `algorithm_kwargs.krum_m`, default n − f): the selected rows, in client-id
  order, are added by `fl.weighted_sum` with unit weights in fp64, divided by m, added to θ_t in
  fp64 and cast once. UNWEIGHTED, as the trimmed mean: a weight would let a client buy influence by
  claiming a large dataset.
"""

from __future__ import annotations

import torch

from ..ops import fl
from ..utils.logging import get_logger
from .robust_algorithm import TrimmedMeanAlgorithm


class MultiKrumAlgorithm(TrimmedMeanAlgorithm):
    track_ids = True
    single: bool = False  # Krum: m = 1

    def __init__(self) -> None:
        super().__init__()
        self.last_selected: list[int] = []  # client ids of the last aggregation's selection
        self.last_scores: dict[int, float] = {}  # client id -> Krum score
        self.last_dists: torch.Tensor | None = None  # the [n, n] fp64 distances
        self.last_ids: list[int] = []  # client id of each row of the last aggregation

    def _kw(self, key: str, default):
        kw = self.config.algorithm_kwargs if self.config is not None else {}
        v = kw.get(key, None)
        return default if v is None else v

    def krum_f(self) -> int:
        return int(self._kw("krum_f", self._kw("byzantine_number", 0)) or 0)

    def krum_m(self, n: int, f: int) -> int:
        return 1 if self.single else int(self._kw("krum_m", n - f))

    def _aggregate(self, old: torch.Tensor) -> torch.Tensor:
        kind = self._kind or self.expected_kind
        rows = self._gather_rows()
        ids = self._round_ids
        n = rows.shape[0]
        self.last_selected, self.last_scores, self.last_dists, self.last_ids = [], {}, None, list(ids)
        if n == 0:
            get_logger().warning("round without any weighted client upload: global model unchanged")
            new = old
        else:
            assert len(ids) == n, (len(ids), n)
            D = fl.pairwise_sq_dists(rows)
            scores, f = fl.krum_scores(D, self.krum_f())
            sel = fl.krum_select(D, f, self.krum_m(n, f), ids)
            self.last_dists = D
            self.last_selected = [ids[i] for i in sel]
            self.last_scores = {ids[i]: float(scores[i]) for i in range(n)}
            get_logger().info("krum: selected clients %s of %d (f = %d)", self.last_selected, n, f)
            if self.single:
                upd = rows[sel[0]].double()
            else:
                picked = rows[torch.tensor(sel, device=rows.device)]
                ones = torch.ones(len(sel), dtype=torch.float64, device=rows.device)
                upd = fl.weighted_sum(picked, ones) / float(len(sel))
            new = old + upd if kind == "delta" else upd
        self.last_trim = (n, 0)
        return new


class KrumAlgorithm(MultiKrumAlgorithm):
    """Krum: Multi-Krum with m = 1."""

    single = True
