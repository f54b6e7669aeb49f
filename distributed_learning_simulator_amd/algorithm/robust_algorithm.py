"""Robust aggregation: coordinate-wise trimmed mean and median (Yin et al. 2018, "Byzantine-robust
distributed learning: towards optimal statistical rates"). Not in the reference, whose every
aggregation is a weighted mean that one NaN, inf or sign-flipped upload destroys.

Per coordinate the n uploads of the round are sorted, the b lowest and b highest dropped and the
rest averaged: `ops.fl.trimmed_sum` (csrc/robust.hip; oracle ops/ref.py), which orders NaNs and
infinities as extreme values, so the trim removes them like any other outlier. The statistic is
UNWEIGHTED: dataset sizes are ignored (a weighted order statistic would let a client buy influence
by claiming a large dataset).

`_process` copies each cohort's dense rows into a round store [n_round, P] on the device (waves
reuse the trainer's buffer). Across ranks the stores are all-gathered (padded to the largest row
count, then compacted), and every rank computes the same result redundantly — the result does not
depend on the row order by construction, so N ranks ≡ 1 rank needs no fixed client order. (Column
sharding with an all-to-all would avoid the redundant pass; it costs about a millisecond.)

b = ⌊trim_ratio · n⌋ (`algorithm_kwargs.trim_ratio`, default 0.1), or (n − 1) // 2 for the median
(the middle value for odd n, the mean of the two middle values for even n). θ_{t+1} = θ_t +
sum/(n − 2b) for delta uploads, sum/(n − 2b) for parameter uploads, in fp64, cast to fp32 once.
"""

from __future__ import annotations

import torch

from ..message import CohortMessage
from ..ops import fl
from ..utils.logging import get_logger
from .aggregation_algorithm import AggregationAlgorithm


class TrimmedMeanAlgorithm(AggregationAlgorithm):
    median: bool = False
    track_ids: bool = False  # Krum: the client ids travel with the rows (`_round_ids`)
    expected_kind: str = "delta"  # set by the session: a rank without clients still knows the kind

    def __init__(self) -> None:
        super().__init__()
        self._store: torch.Tensor | None = None  # [capacity, P] fp32, kept across rounds
        self._n = 0  # rows of this round held by this rank
        self._ids: list[int] = []  # their client ids, in row order
        self._round_ids: list[int] = []  # ids of the rows `_gather_rows` returned (track_ids)
        self._kind: str | None = None
        self.last_trim: tuple[int, int] = (0, 0)  # (n, b) of the last aggregation

    # ------------------------------------------------------------------ round store
    def _reserve(self, rows: int) -> torch.Tensor:
        P = self.layout.padded_size
        if self._store is None or self._store.shape[0] < rows or self._store.device != self.device:
            cap = max(rows, 2 * self._store.shape[0] if self._store is not None else 0)
            new = torch.empty((cap, P), dtype=torch.float32, device=self.device)
            if self._store is not None and self._n:
                new[: self._n].copy_(self._store[: self._n])
            self._store = new
        return self._store

    def _process(self, msg: CohortMessage, old_parameter) -> None:
        if msg.mask is not None or msg.block_mask is not None:
            raise RuntimeError("robust aggregation takes dense uploads (no element or block masks)")
        if self._kind is None:
            self._kind = msg.kind
        if self._kind != msg.kind:
            raise RuntimeError(f"mixed message kinds in one round: {self._kind} vs {msg.kind}")
        rows = msg.dense()
        K = rows.shape[0]
        store = self._reserve(self._n + K)
        store[self._n : self._n + K].copy_(rows)
        self._n += K
        self._ids.extend(int(c) for c in msg.client_ids)

    # ------------------------------------------------------------------ ranks
    def _gather_rows(self) -> torch.Tensor:
        """All ranks' rows of the round as one [n, P]. The per-rank row counts and the host-side
        round flags (end_training, whether a rank carries other_data) ride in one small all-gather;
        with `track_ids` the client ids follow in a second one, padded like the rows."""
        comm, P = self.comm, self.layout.padded_size
        local = self._store[: self._n] if self._n else torch.empty((0, P), dtype=torch.float32, device=self.device)
        self._round_ids = list(self._ids)
        if not comm.is_distributed:
            return local
        head = torch.tensor([self._n, 1 if self._end_training else 0, 1 if self._other_data else 0],
                            dtype=torch.int64, device=self.device)
        heads = torch.stack(comm.all_gather(head)).tolist()
        counts = [int(h[0]) for h in heads]
        self._merge_round_flags(any(h[1] for h in heads), any(h[2] for h in heads))
        m = max(counts)
        if m == 0:
            return local
        if self.track_ids:
            ids = torch.full((m,), -1, dtype=torch.int64, device=self.device)
            ids[: self._n] = torch.tensor(self._ids, dtype=torch.int64, device=self.device)
            self._round_ids = [int(c) for p, k in zip(comm.all_gather(ids), counts) for c in p[:k].tolist()]
        padded = torch.zeros((m, P), dtype=torch.float32, device=self.device)
        padded[: self._n].copy_(local)
        parts = comm.all_gather(padded)
        if all(c == m for c in counts):
            return torch.cat(parts)
        return torch.cat([p[:c] for p, c in zip(parts, counts) if c])

    def trim(self, n: int) -> int:
        """Rows dropped at each end for n uploads."""
        med = (n - 1) // 2
        if self.median:
            return med
        ratio = float(self.config.algorithm_kwargs.get("trim_ratio", 0.1)) if self.config is not None else 0.1
        b = int(ratio * n)
        if b < 0 or 2 * b >= n:
            get_logger().warning("trim_ratio %s leaves no upload of %d: falling back to the median", ratio, n)
            return med
        return b

    def _aggregate(self, old: torch.Tensor) -> torch.Tensor:
        kind = self._kind or self.expected_kind
        rows = self._gather_rows()
        n = rows.shape[0]
        if n == 0:
            # every selected client failed / skipped: keep θ_t
            get_logger().warning("round without any weighted client upload: global model unchanged")
            new, b = old, 0
        else:
            b = self.trim(n)
            mean = fl.trimmed_sum(rows, b) / float(n - 2 * b)
            new = old + mean if kind == "delta" else mean
        self.last_trim = (n, b)
        return new

    def _reset_round(self) -> None:
        self._n = 0
        self._ids = []
        self._kind = None


class MedianAlgorithm(TrimmedMeanAlgorithm):
    """Coordinate-wise median: the trimmed mean with b = (n − 1) // 2."""

    median = True
