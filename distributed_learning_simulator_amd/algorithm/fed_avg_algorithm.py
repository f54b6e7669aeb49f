"""FedAvg (dataset-size weighted), cohort form.

Reference `algorithm/fed_avg_algorithm.py:11-110`: streaming accumulation of
float64(θ_k)·n_k and Σ n_k, finalize θ = (acc/W).to(dtype), NaN assert, `end_training` from
the first worker, merged `other_data`. Delta uploads are restored against θ_t first
(`aggregation_algorithm.py:52-71`), i.e. θ_{t+1} = θ_t + Σ n_kΔ_k / Σ n_k.

MI355X-native execution: per cohort ONE fused `weighted_sum` kernel
over [K, P] adding into an fp64 accumulator (the reference's float64 invariant holds across
cohorts AND ranks) → after all local cohorts ONE fp64 `all_reduce(SUM)` of the accumulator and
weights across ranks (RCCL over xGMI; 2× the bytes of fp32, still ≈0.1 ms for ResNet-18) →
finalize in fp64, cast to fp32 once. The result is already resident on every rank, so the
broadcast M5 needs no second collective. A round in which no selected client reported (every
one failed) leaves the global model unchanged.

Generalisations used by the methods:
* element masks (`msg.mask`, FedDropoutAvg) → per-element weights (`_get_weight` analogue);
* block masks (`msg.block_mask`, FedOBD stage 1) → per-block weights: a block is averaged
  over the clients that sent it; blocks no client sent keep θ_t (fixes B4).

The round's frame (θ_t → fp64, `last_fp64`, the one cast, the NaN assertion, the result
message, the reset) is `AggregationAlgorithm.aggregate_worker_data`; this class fills in
`_process`, `_aggregate` and `_reset_round`. A method built on the fp64 accumulator (DP-FedAvg,
secure aggregation, SCAFFOLD) overrides `_process` and `_aggregate`, calls `_ensure_acc()` and
`_reduce()` for the accumulator and the cross-rank sum, and extends `_reset_round`.
"""

from __future__ import annotations

import torch

from ..message import CohortMessage
from ..ops import fl
from ..utils.logging import get_logger
from .aggregation_algorithm import AggregationAlgorithm


class FedAVGAlgorithm(AggregationAlgorithm):
    def __init__(self) -> None:
        super().__init__()
        self.accumulate: bool = True
        self._acc: torch.Tensor | None = None
        self._w_total: torch.Tensor | None = None  # scalar [1]
        self._w_elem: torch.Tensor | None = None  # [P] (element masks)
        self._w_block: torch.Tensor | None = None  # [nblocks] (block masks)
        self._block_ids: torch.Tensor | None = None
        self._kind: str | None = None
        self._dataset_size = 0.0
        self._reported = 0  # clients whose upload this round's accumulator holds (all ranks after _reduce)

    # weights hook (reference `_get_weight`): dataset size
    def _weights(self, msg: CohortMessage) -> torch.Tensor:
        return msg.dataset_sizes.to(self.device, torch.float64)

    def _process(self, msg: CohortMessage, old_parameter) -> None:
        self.expected_kind = msg.kind if self._acc is None else self.expected_kind
        self._ensure_acc()
        if self._kind != msg.kind:
            raise RuntimeError(f"mixed message kinds in one round: {self._kind} vs {msg.kind}")
        w = self._weights(msg)
        if msg.mask is not None:
            if self._w_elem is None:
                self._w_elem = torch.zeros_like(self._acc)
            fl.masked_weighted_sum(msg.dense(), msg.mask, w, self._acc, self._w_elem)
        else:
            if msg.payload is not None:  # packed upload: dequantised inside the fp64 accumulation
                msg.payload.accumulate(self._acc, w)
            else:
                fl.weighted_sum(msg.dense(), w, self._acc)
            if msg.block_mask is not None:
                bw = (msg.block_mask.double() * w[:, None]).sum(0)
                self._w_block = bw if self._w_block is None else self._w_block + bw
                self._block_ids = msg.extra["block_ids"]
        self._w_total += w.sum()
        # clients that carry weight: counted on the host when the sizes are host tensors; a
        # device-resident size vector is not read back (no sync per message), so there every
        # message's clients count and the 'no reported client' warning means 'no upload'
        ds = msg.dataset_sizes
        self._reported += int((ds != 0).sum()) if not ds.is_cuda else len(msg.client_ids)
        self._dataset_size += float(msg.dataset_sizes.sum().item()) if not msg.dataset_sizes.is_cuda else 0.0

    @property
    def fuses_payload(self) -> bool:
        """Packed uploads are dequantised inside `_process` (not decoded by the endpoint) unless
        a subclass replaces `_process`."""
        return type(self)._process is FedAVGAlgorithm._process

    # set by the method/session so that a rank hosting no client this round still joins the
    # collectives with correctly shaped (zero) contributions
    expected_kind: str = "delta"
    expects_element_mask: bool = False
    num_blocks: int = 0
    block_ids: torch.Tensor | None = None

    def _ensure_acc(self) -> None:
        P = self.layout.padded_size
        if self._acc is None:
            self._acc = torch.zeros(P, dtype=torch.float64, device=self.device)
            self._w_total = torch.zeros(1, dtype=torch.float64, device=self.device)
            self._kind = self.expected_kind
        if self.expects_element_mask and self._w_elem is None:
            self._w_elem = torch.zeros(P, dtype=torch.float64, device=self.device)
        if self.num_blocks and self._w_block is None:
            self._w_block = torch.zeros(self.num_blocks, dtype=torch.float64, device=self.device)
            self._block_ids = self.block_ids

    def _reduce(self) -> None:
        """fp64 accumulator + weights summed over ranks. The host-side round flags (end_training,
        whether any rank carries other_data, how many clients reported) ride in the same small
        all-reduce, read with ONE host transfer; the pickled all_gather_object runs only in a
        round where some rank actually has other_data to merge."""
        comm = self.comm
        small = [self._w_total] + ([self._w_block] if self._w_block is not None else [])
        flags = None
        if comm.is_distributed:
            flags = torch.tensor([1.0 if self._end_training else 0.0, 1.0 if self._other_data else 0.0,
                                  float(self._reported)], dtype=torch.float64, device=self.device)
            small.append(flags)
        comm.all_reduce_(self._acc)
        comm.all_reduce_many_(small)
        if self._w_elem is not None:
            comm.all_reduce_(self._w_elem)
        if flags is not None:
            end, other, reported = flags.tolist()
            self._reported = int(reported)
            self._merge_round_flags(end > 0, other > 0)

    def _aggregate(self, old: torch.Tensor) -> torch.Tensor:
        self._ensure_acc()
        self._reduce()
        acc = self._acc
        zero = torch.zeros((), dtype=torch.float64, device=self.device)
        if self._w_elem is not None:
            den = self._w_elem
            if self._kind == "delta":
                new = torch.where(den > 0, old + acc / den.clamp(min=1e-300), old)
            else:
                # reference `fed_dropout_avg/algorithm.py:9-18`: zero total weight -> 1
                new = acc / torch.where(den == 0, torch.ones_like(den), den)
        elif self._w_block is not None:
            wb = self._w_block
            ids = self._block_ids.long()
            we = torch.where(ids >= 0, wb[ids.clamp(min=0)], zero)
            if self._kind == "delta":
                new = torch.where(we > 0, old + acc / we.clamp(min=1e-300), old)
            else:
                new = torch.where(we > 0, acc / we.clamp(min=1e-300), old)
        else:
            wt = self._w_total
            # every selected client failed / skipped: keep θ_t (no 0/0 NaN model)
            if self._kind == "delta":
                new = torch.where(wt > 0, old + acc / wt.clamp(min=1e-300), old)
            else:
                new = torch.where(wt > 0, acc / wt.clamp(min=1e-300), old)
            if self._reported == 0:  # (host-side count: no device read)
                get_logger().warning("round without any weighted client upload: global model unchanged")
        return new

    def _reset_round(self) -> None:
        self._reported = 0
        self._acc = None
        self._w_total = None
        self._w_elem = None
        self._w_block = None
        self._kind = None
