"""Secure aggregation with pairwise masks (Bonawitz et al., CCS 2017; sparse mask graphs: Bell et al., CCS
2020): the server adds uploads it cannot read and unmasks only their sum. Not in the reference.

WHAT IS SIMULATED. The protocol's dataflow, arithmetic, failure handling and cost. Philox is not a
cryptographic generator, the key agreement runs in a toy group and all parties live in one process:
`fed_secagg` gives no security to anybody. It shows what a deployment computes, moves and pays.

Per upload message `_process` accepts only a `MaskedPayload` (worker/secagg_worker.py) and adds its int32
rows into an int64 accumulator (`ops.fl.ring_sum`, csrc/secagg.hip; 8 · P bytes, the size of FedAvg's fp64
one). `aggregate_worker_data`: one `all_gather_object` of the reporting client ids (with the simulator's
clamp / NaN counters), one int64 all-reduce of the accumulator, then every rank runs the same recovery
(utils/secagg_protocol.py — keyed by (seed, round), so no further collective): the self masks of the clients
that reported and the pair masks of those that dropped are rebuilt from Shamir shares and removed with
`ops.fl.ring_unmask`; `ops.fl.ring_decode` gives Σ_S q(Δ_c) · 2^−f exactly and

    θ_{t+1} = θ_t + decoded / |S|        in fp64, cast once

— the UNWEIGHTED mean over the clients that reported (a weight would have to be applied before masking).
If a secret cannot be rebuilt (fewer than t shares among the reporting clients) the round aborts: θ is
unchanged and `secagg_aborted` = 1. A round in which nobody reported leaves θ unchanged too. Every value
is an integer of Z_{2^32}: any number of ranks, waves and resumed runs give the same bits.

`algorithm_kwargs`: `secagg_range` R (required, finite, > 0: deltas are clamped to [−R, R]), `secagg_frac_bits`
f (default: the largest with m · R · 2^f ≤ 2^31 − 1, m the fixed cohort size — `random_client_number` if set,
else `worker_number`), `secagg_degree` (0: complete graph, else even), `secagg_threshold` (default d // 2 + 1).
`round_stats`: `secagg_survivors`, `secagg_dropped`, `secagg_aborted`, `secagg_clamped_fraction` (over the
reporting clients' valid elements), `secagg_nan_elements`, `secagg_frac_bits`, `secagg_mask_streams` (Σ_S (d_c
+ 1) client-side streams plus the server's unmask entries), `secagg_dropped_bytes` (Σ_D 16 + 32 · d_x: what
the dropped clients had sent; not part of `comm_bytes_up`). `last_fp64` is set: a `server_optimizer` works
behind it unchanged.
"""

from __future__ import annotations

import torch

from ..config import clients_per_round
from ..message import CohortMessage
from ..ops import compress, fl
from ..utils.logging import get_logger
from ..utils.secagg_protocol import mask_graph, round_protocol
from .fed_avg_algorithm import FedAVGAlgorithm


def cohort_size(config) -> int:
    """The fixed m: `random_client_number` if set, else `worker_number`."""
    return clients_per_round(config.algorithm_kwargs, config.worker_number)


def secagg_settings(config) -> tuple[float, int, int, int | None]:
    """(R as fp32, f, degree, threshold or None) from `algorithm_kwargs`; ValueError on bad values."""
    kw = config.algorithm_kwargs
    if kw.get("secagg_range") is None:
        raise ValueError("fed_secagg: algorithm_kwargs.secagg_range is required")
    m = cohort_size(config)
    R, f = fl.secagg_frac_bits(kw["secagg_range"], m, kw.get("secagg_frac_bits"))
    try:
        degree = int(kw.get("secagg_degree") or 0)
        threshold = None if kw.get("secagg_threshold") is None else int(kw["secagg_threshold"])
    except (TypeError, ValueError) as e:
        raise ValueError(f"fed_secagg: secagg_degree and secagg_threshold must be integers ({e})") from e
    partners = mask_graph(range(m), degree)  # (raises on an odd or negative degree)
    d = len(partners[0])
    if threshold is not None and d and not 1 <= threshold <= d:
        raise ValueError(f"fed_secagg: secagg_threshold {threshold} outside [1, {d}] (the mask graph's degree)")
    return R, f, degree, threshold


class SecAggAlgorithm(FedAVGAlgorithm):
    def __init__(self) -> None:
        super().__init__()
        self.range, self.frac_bits, self.degree, self.threshold = 1.0, 1, 0, None
        self._ids: list[int] = []  # this round's reporting clients on this rank, in upload order
        self._counters: list[torch.Tensor] = []  # ... and their (clamped, NaN) counters, one tensor per message
        self._valid = 0
        self.last_reporting: list[int] = []
        self.last_dropped: list[int] = []

    def bind(self, config, layout, device, comm=None, server=None) -> None:
        super().bind(config, layout, device, comm, server)
        self.range, self.frac_bits, self.degree, self.threshold = secagg_settings(config)
        self._valid = int(layout.num_params)

    def _selected(self) -> list[int]:
        return list(self.server.selected) if self.server is not None else sorted(self.last_reporting)

    @property
    def fuses_payload(self) -> bool:
        return True  # the endpoint must not try to decode a masked upload

    def _ensure_acc(self) -> None:
        if self._acc is None:
            self._acc = torch.zeros(self.layout.padded_size, dtype=torch.int64, device=self.device)
            self._w_total = torch.zeros(1, dtype=torch.float64, device=self.device)
            self._kind = "delta"

    def _process(self, msg: CohortMessage, old_parameter) -> None:
        if msg.mask is not None or msg.block_mask is not None:
            raise RuntimeError("fed_secagg takes masked fixed-point uploads: no element or block masks")
        if msg.kind != "delta":
            raise RuntimeError(f"fed_secagg masks client deltas: delta uploads only, got kind {msg.kind!r}")
        if not isinstance(msg.payload, compress.MaskedPayload):
            raise RuntimeError("fed_secagg takes MaskedPayload uploads only (SecAggWorker, plain endpoints), got "
                               f"{'dense rows' if msg.payload is None else type(msg.payload).__name__}")
        self.expected_kind = "delta"
        self._ensure_acc()
        msg.payload.accumulate(self._acc)
        self._ids.extend(int(c) for c in msg.client_ids)
        self._counters.append(msg.extra["secagg_stats"])
        self._reported += len(msg.client_ids)

    def _aggregate(self, old: torch.Tensor) -> torch.Tensor:
        if self.expected_kind != "delta":
            raise RuntimeError("fed_secagg masks client deltas: the workers must upload parameter differences")
        self._ensure_acc()
        # client id -> (clamped, NaN) over all ranks: one host read of this rank's counters, one gather
        reports = self._gather_client_values(self._ids, self._counters)
        self._reduce()  # one int64 all-reduce of the accumulator (+ the round flags)
        S = sorted(reports)
        selected = sorted(set(self._selected()) | set(S))
        proto = round_protocol(self.config.seed, self.round_index(), selected, self.degree, self.threshold)
        D = [c for c in proto.ids if c not in reports]
        keys, signs, aborted = proto.recover(S)
        if aborted:
            get_logger().warning("fed_secagg: round %d aborted, too few shares survive (reporting %s, dropped %s): "
                                 "global model unchanged", self.round_index(), S, D)
            new = old.clone()
        elif not S:
            get_logger().warning("round without any client upload: global model unchanged")
            new = old.clone()
        else:
            fl.ring_unmask(self._acc, (keys, signs))
            dec = fl.ring_decode(self._acc, self.frac_bits)
            new = old + dec / torch.full((), float(len(S)), dtype=torch.float64, device=self.device)
        clamped = sum(v[0] for v in reports.values())
        self.last_reporting, self.last_dropped = S, D
        self.round_stats = {
            "secagg_survivors": len(S),
            "secagg_dropped": len(D),
            "secagg_aborted": int(aborted),
            "secagg_clamped_fraction": clamped / (len(S) * self._valid) if S and self._valid else 0.0,
            "secagg_nan_elements": sum(v[1] for v in reports.values()),
            "secagg_frac_bits": self.frac_bits,
            "secagg_mask_streams": sum(len(proto.client_entries(c)) for c in S) + len(keys),
            "secagg_dropped_bytes": sum(proto.dropped_bytes(c) for c in D),
        }
        return new

    def _reset_round(self) -> None:
        super()._reset_round()
        self._ids = []
        self._counters = []
