"""Client-level DP-FedAvg (McMahan et al. 2018, "Learning differentially private recurrent language
models"): every client's update is clipped to an L2 norm C and Gaussian noise of std z · C is added
to the sum. Not in the reference.

Per upload message `_process` runs `ops.fl.row_sq_norms` (fp64 squared norms of the dense delta rows,
fixed summation order) and `ops.fl.clipped_sum` (rows scaled by min(1, C / norm) and added in fp64 into
the FedAvg accumulator; the factors are formed on the device, NaN / inf rows are rejected) —
csrc/dp.hip, oracle ops/ref.py. The norms stay on the device until the round is aggregated.

`aggregate_worker_data`: one fp64 all-reduce of the accumulator (`FedAVGAlgorithm._reduce`), then
every rank adds the same noise, `ops.fl.gaussian_add(acc, z · C, config.seed, round, valid_mask)` —
Philox keyed by (seed, round), so it needs no state, is the same on every rank and survives a
checkpoint — and θ_{t+1} = θ_t + acc / m in fp64, cast once.

* Clients are UNWEIGHTED: a dataset-size weight would scale a client's contribution past C and
  break the sensitivity bound.
* The denominator m is FIXED: `random_client_number` if set, else `worker_number`. It does not
  shrink when clients fail or are rejected — a data-dependent denominator would leak, and the
  noise std on the mean is z · C / m as accounted.

`algorithm_kwargs`: `dp_clip_norm` (required, > 0), `dp_noise_multiplier` (z, default 1.0; 0 = clipping
only, no noise is drawn), `dp_delta` (default 1e-5). Per round `round_stats` (merged into the
session's metrics row) holds `dp_clipped_fraction`, `dp_median_norm`, `dp_rejected`, `dp_epsilon` —
the unamplified composition of the rounds so far, valid for any participation scheme — and
`dp_epsilon_poisson`, amplified at q = m / worker_number, which would hold only if clients were
Poisson-sampled: the simulator draws a fixed-size subset, so it is indicative, not a guarantee
(`utils/privacy.py`).
"""

from __future__ import annotations

import math
import statistics

import torch

from ..config import clients_per_round
from ..message import CohortMessage
from ..ops import fl
from ..utils import privacy
from ..utils.logging import get_logger
from .fed_avg_algorithm import FedAVGAlgorithm


def dp_settings(config) -> tuple[float, float, float]:
    """(clip norm C, noise multiplier z, δ) from `algorithm_kwargs`; ValueError on bad values."""
    kw = config.algorithm_kwargs
    if kw.get("dp_clip_norm") is None:
        raise ValueError("fed_dp_avg: algorithm_kwargs.dp_clip_norm is required")
    try:
        clip = float(kw["dp_clip_norm"])
        z = float(1.0 if kw.get("dp_noise_multiplier") is None else kw["dp_noise_multiplier"])
        delta = float(1e-5 if kw.get("dp_delta") is None else kw["dp_delta"])
    except (TypeError, ValueError) as e:
        raise ValueError(f"fed_dp_avg: dp_clip_norm, dp_noise_multiplier and dp_delta must be numbers ({e})") from e
    if not (clip > 0.0 and math.isfinite(clip)):
        raise ValueError(f"fed_dp_avg: dp_clip_norm must be a finite positive number, got {clip}")
    if not (z >= 0.0 and math.isfinite(z)):
        raise ValueError(f"fed_dp_avg: dp_noise_multiplier must be a finite number >= 0, got {z}")
    if not 0.0 < delta < 1.0:
        raise ValueError(f"fed_dp_avg: dp_delta must lie in (0, 1), got {delta}")
    return clip, z, delta


class DPFedAvgAlgorithm(FedAVGAlgorithm):
    def __init__(self) -> None:
        super().__init__()
        self.clip, self.noise_multiplier, self.delta = 1.0, 1.0, 1e-5
        self._nsq: list[torch.Tensor] = []  # this round's squared norms, one device tensor per message
        self._ids: list[int] = []  # ... and the client ids, in the same order
        self._rdp: tuple[list[float], list[float]] | None = None  # RDP curves at q = 1 and q = m / N
        self._mask: torch.Tensor | None = None
        self.last_norms: dict[int, float] = {}  # client id -> L2 norm of its upload (all ranks)
        self.last_clipped: list[int] = []  # client ids whose upload was scaled down
        self.last_rejected: list[int] = []  # client ids whose upload was not finite
        self.last_acc: torch.Tensor | None = None  # the fp64 accumulator after the noise

    def bind(self, config, layout, device, comm=None, server=None) -> None:
        super().bind(config, layout, device, comm, server)
        self.clip, self.noise_multiplier, self.delta = dp_settings(config)
        self._rdp = None
        self._mask = None

    # ------------------------------------------------------------------ settings
    def denominator(self) -> int:
        """The fixed m of the mean: `random_client_number` if set, else `worker_number`."""
        return clients_per_round(self.config.algorithm_kwargs, self.config.worker_number)

    def _valid_mask(self) -> torch.Tensor | None:
        if self._mask is None and hasattr(self.layout, "valid_mask"):
            self._mask = self.layout.valid_mask(self.device).to(torch.uint8)
        return self._mask

    def epsilons(self, rounds: int) -> tuple[float, float]:
        """(ε of `rounds` unamplified compositions, ε with Poisson amplification at q = m / N)."""
        z = self.noise_multiplier
        if z == 0.0:
            return math.inf, math.inf
        if self._rdp is None:
            q = self.denominator() / float(self.config.worker_number)
            self._rdp = (privacy.rdp_curve(z, 1.0), privacy.rdp_curve(z, q))
        return (privacy.epsilon_from_rdp(self._rdp[0], rounds, self.delta),
                privacy.epsilon_from_rdp(self._rdp[1], rounds, self.delta))

    # ------------------------------------------------------------------ round
    @property
    def fuses_payload(self) -> bool:
        return False

    def _process(self, msg: CohortMessage, old_parameter) -> None:
        if msg.mask is not None or msg.block_mask is not None or msg.payload is not None:
            raise RuntimeError("fed_dp_avg takes dense delta uploads (no element or block masks, no packed payloads)")
        if msg.kind != "delta":
            raise RuntimeError(f"fed_dp_avg clips client deltas: dense delta uploads only, got kind {msg.kind!r}")
        self.expected_kind = "delta"
        self._ensure_acc()
        rows = msg.dense()
        nsq = fl.row_sq_norms(rows)
        fl.clipped_sum(rows, nsq, self.clip, self._acc)
        self._nsq.append(nsq)
        self._ids.extend(int(c) for c in msg.client_ids)
        self._reported += len(msg.client_ids)

    def _aggregate(self, old: torch.Tensor) -> torch.Tensor:
        if self.expected_kind != "delta":
            raise RuntimeError("fed_dp_avg clips client deltas: the workers must upload parameter differences")
        self._ensure_acc()
        self._reduce()
        acc, rnd, m = self._acc, self.round_index(), self.denominator()
        # client id -> squared norm over all ranks: ONE host read of this rank's n doubles
        nsq = {c: v for c, (v,) in self._gather_client_values(self._ids, self._nsq).items()}
        self.last_rejected = [c for c, v in nsq.items() if not math.isfinite(v)]
        self.last_norms = {c: math.sqrt(v) if math.isfinite(v) and v >= 0.0 else math.nan for c, v in nsq.items()}
        self.last_clipped = [c for c, v in self.last_norms.items() if v > self.clip]
        if self.last_rejected:
            get_logger().warning("fed_dp_avg: rejected the non-finite uploads of clients %s", self.last_rejected)
        if self.noise_multiplier > 0.0:  # the same draw on every rank: keyed by (seed, round, position)
            fl.gaussian_add(acc, self.noise_multiplier * self.clip, int(self.config.seed), rnd, self._valid_mask())
        new = old + acc / torch.full((), float(m), dtype=torch.float64, device=self.device)
        if not nsq:
            get_logger().warning("round without any client upload: the global model moves by the noise alone")
        finite = [v for v in self.last_norms.values() if math.isfinite(v)]
        eps, eps_poisson = self.epsilons(rnd)
        self.round_stats = {
            "dp_clipped_fraction": len(self.last_clipped) / len(nsq) if nsq else 0.0,
            "dp_median_norm": float(statistics.median(finite)) if finite else 0.0,
            "dp_rejected": len(self.last_rejected),
            "dp_epsilon": eps,
            "dp_epsilon_poisson": eps_poisson,
        }
        self.last_acc = acc
        return new

    def _reset_round(self) -> None:
        super()._reset_round()
        self._nsq = []
        self._ids = []
