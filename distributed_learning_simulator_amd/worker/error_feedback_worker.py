"""Update sparsification with error feedback.

Reference `worker/error_feedback_worker.py:9-19`: an abstract AggregationWorker that
requires diff uploads (`send_parameter_diff`), keeps an `_error` residual and leaves
`sparsify()` unimplemented (no concrete subclass in the reference tree).

Here the residual is a per-client row of a device buffer: each round a client uploads
S(Δ + e) and keeps e ← (Δ + e) − S(Δ + e). The residual lives on the rank that trains the
client, so the client→rank assignment must be stable across rounds (full participation, or
one rank). `TopKErrorFeedbackWorker` is a concrete sparsifier (largest-|x| fraction per
client row; wire bytes = k values + k int32 indices). `PackedTopKWorker` (method `fed_topk`) is
the full form: an exact, tie-ordered selection by the hand-written kernels of csrc/topk.hip into
a packed `ops.compress.SparsePayload` that the server accumulates directly; no dense sparse
rows exist on the client side. `RotSignWorker` (method `fed_drive`) uploads one sign bit per
coordinate of a randomised Hadamard rotation (csrc/rotsign.hip), with or without the residual.
"""

from __future__ import annotations

import torch

from ..config import clients_per_round
from ..message import CohortMessage
from ..ops import compress, fl
from .aggregation_worker import AggregationWorker


class ErrorFeedbackWorker(AggregationWorker):
    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        assert self._send_parameter_diff, "error feedback needs delta uploads"
        self._error: torch.Tensor | None = None  # [worker_number, P_pad] residuals
        self._meta: compress.LayoutMeta | None = None  # (packed uploads: `_layout_meta`)

    def state_dict(self) -> dict:
        return {"error": self._error.cpu()} if self._error is not None else {}

    def load_state_dict(self, state: dict) -> None:
        if "error" in state:
            self._error = state["error"].to(self.trainer.buffers.theta.device)

    def sparsify(self, rows: torch.Tensor) -> tuple[torch.Tensor, list[int]]:
        """rows [K,P] (Δ + e) → (sparse rows [K,P] with zeros where not sent, wire bytes per row)."""
        raise NotImplementedError

    def _ensure_error(self, P: int, device) -> torch.Tensor:
        if self._error is None:
            W = self.config.worker_number
            sel = clients_per_round(self.config.algorithm_kwargs, W)
            world = self.session.comm.world if self.session is not None else 1
            assert sel >= W or world == 1, "error feedback residuals need a stable client→rank assignment"
            self._error = torch.zeros((W, P), dtype=torch.float32, device=device)
        return self._error

    def _error_rows(self, wave: list[int], P: int, device) -> torch.Tensor:
        return self._ensure_error(P, device)[torch.tensor(wave, device=device)]

    # ------------------------------------------------------------------ packed uploads
    def _layout_meta(self, device) -> compress.LayoutMeta:
        if self._meta is None or self._meta.seg_ids.device != device:
            self._meta = compress.LayoutMeta.of(self.trainer.layout, device)
        return self._meta

    def _pack_with_residual(self, wave: list[int], rows: torch.Tensor, pack):
        """`pack(rows, err)` over the wave's residual rows err [K, P], which it updates: in place when
        the wave's clients are consecutive rows of `_error`, else gathered, packed and scattered back."""
        K, P = rows.shape
        error = self._ensure_error(P, rows.device)
        if list(wave) == list(range(wave[0], wave[0] + K)):
            return pack(rows, error[wave[0] : wave[0] + K])
        idx = torch.tensor(wave, device=rows.device)
        err = error[idx]
        payload = pack(rows, err)
        error[idx] = err
        return payload

    def _get_sent_data(self, wave, theta_g, stats) -> CohortMessage:
        msg = super()._get_sent_data(wave, theta_g, stats)
        rows = msg.data
        idx = torch.tensor(wave, device=rows.device)
        rows += self._error_rows(wave, rows.shape[1], rows.device)
        sparse, nbytes = self.sparsify(rows)
        self._error[idx] = rows - sparse
        rows.copy_(sparse)
        msg.extra["wire_bytes"] = list(nbytes)
        return msg


class TopKErrorFeedbackWorker(ErrorFeedbackWorker):
    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        self.ratio = float(config.algorithm_kwargs.get("topk_ratio", 0.01))

    def sparsify(self, rows):
        n = self.trainer.layout.num_params
        k = max(1, int(n * self.ratio))
        valid = self.trainer.layout.valid_mask(rows.device)
        mag = rows.abs().masked_fill(~valid, -1.0)
        top = mag.topk(k, dim=1).indices
        out = torch.zeros_like(rows)
        out.scatter_(1, top, rows.gather(1, top))
        return out, [k * 8] * rows.shape[0]


class PackedTopKWorker(ErrorFeedbackWorker):
    """Top-k error feedback with a packed upload: `ops.compress.pack_topk_ef` selects from
    Δ + e, writes the (idx, val) payload and leaves the residual e ← (Δ + e) − S(Δ + e) in
    `_error`, in place when the wave's clients are consecutive rows of it."""

    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        self.ratio = float(config.algorithm_kwargs.get("topk_ratio", 0.01))

    def topk(self) -> int:
        return max(1, int(self.trainer.layout.num_params * self.ratio))

    def _get_sent_data(self, wave, theta_g, stats) -> CohortMessage:
        msg = AggregationWorker._get_sent_data(self, wave, theta_g, stats)
        meta, k = self._layout_meta(msg.data.device), self.topk()
        payload = self._pack_with_residual(wave, msg.data, lambda rows, err: compress.pack_topk_ef(rows, err, meta, k))
        return self._attach_payload(msg, payload, payload.row_bytes())


class RotSignWorker(ErrorFeedbackWorker):
    """1-bit rotated uploads (method `fed_drive`, csrc/rotsign.hip): every client sends the sign bits
    of the randomised Hadamard rotation of its delta and one fp32 scale per 4096-element block
    (`ops.compress.RotSignPayload`). `algorithm_kwargs.error_feedback`:
    - false (default): DRIVE's unbiased scale, no client state, so partial participation works;
    - true: the MSE-optimal scale with the residual e ← (Δ + e) − x̂ kept in `_error`, which needs
      the stable client→rank assignment of every error-feedback worker.
    The rotation's diagonal is keyed by (round's upload seed, client id): it changes every round and
    does not depend on which rank or row hosts a client."""

    def __init__(self, config, endpoint, session=None, **kwargs):
        super().__init__(config, endpoint, session, **kwargs)
        self.error_feedback = bool(config.algorithm_kwargs.get("error_feedback", False))

    def _get_sent_data(self, wave, theta_g, stats) -> CohortMessage:
        msg = AggregationWorker._get_sent_data(self, wave, theta_g, stats)
        meta = self._layout_meta(msg.data.device)
        seeds = fl.row_seeds(self.upload_seed(self._round_num), list(wave))
        if not self.error_feedback:  # (no residual: `_error` is never allocated)
            payload = compress.pack_rotsign(msg.data, meta, seeds, scale="unbiased")
        else:
            payload = self._pack_with_residual(wave, msg.data,
                                               lambda rows, err: compress.pack_rotsign_ef(rows, err, meta, seeds))
        return self._attach_payload(msg, payload, payload.row_bytes())
