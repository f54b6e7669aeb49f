"""Materialised compressed payloads: the wire buffers quantising endpoints actually send.

Reference `topology/quantized_endpoint.py:29-34,58-68,86-116`: the client endpoint REPLACES the
uploaded tensors with their quantised form and the server dequantises what it receives;
`get_message_size` then counts the quantised tensors. Here the quantiser writes one ragged
uint8 buffer per cohort:
- client k's bytes start at `row_off[k]`;
- tensor s of client k occupies ceil(bits·numel / 8) bytes at `seg_byte_off[k, s]`, with b-bit
  codes packed LSB-first in 8-element groups (csrc/compress.hip);
- per sent tensor there is the fp32 norm (stochastic) or fp32 `lo` and `scale` + one uint8
  bit-width (NNADQ).

Wire bytes per client are the sizes of those buffers (`QuantPayload.row_bytes`), not a formula.
The server either decodes to dense rows or, for FedAvg-style weighted sums, dequantises inside
the fp64 accumulation kernel (`accumulate`: no dense [K, P] materialisation).

`SparsePayload` (fed_topk, csrc/topk.hip) is the sparse member of the family: per client the k
largest-|u| elements as int32 indices + fp32 values, 8k bytes, with the same decode / accumulate
interface; `pack_topk_ef` also keeps the error-feedback residual.

Codes:
- stochastic (FedPAQ / fed_obd_sq, QSGD with 255 signed levels = 8 bits, ops.quant): lo = −‖x‖,
  scale = ‖x‖/127, q = clamp(floor((x − lo)/scale + u), 0, 254), with u the shared per-element
  hash uniform (`fl.uniform_rows`; unbiased); per sent tensor only the fp32 norm travels;
- NNADQ (FedOBD): round-to-nearest with the per-tensor adaptive bit-width of `quant.nnadq_bits`.

x̂ = lo + q·scale; the CPU path below writes the identical buffer and decodes to identical bits.

`RotSignPayload` (fed_drive, csrc/rotsign.hip) is the 1-bit member (DRIVE / EDEN): per client and per
block of 4096 flat elements the sign bits of a randomised Hadamard rotation and one fp32 scale, 516
bytes per block, with the same decode / accumulate interface; `pack_rotsign_ef` keeps the residual.

`MaskedPayload` (fed_secagg, csrc/secagg.hip) carries the masked fixed-point rows of secure aggregation:
int32 words that only add up (`accumulate` into an int64 ring accumulator); there is no dense form to decode.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from . import backend, ref
from .fl import _mix, uniform_rows


@dataclass
class LayoutMeta:
    seg_ids: torch.Tensor  # int32 [P] (padding = nseg)
    seg_off: torch.Tensor  # int64 [nseg] flat offsets (16-element aligned)
    seg_numel: torch.Tensor  # int64 [nseg]
    nseg: int
    P: int
    _vbits: torch.Tensor | None = None
    _num_params: int = -1

    @property
    def num_params(self) -> int:
        if self._num_params < 0:
            self._num_params = int(self.seg_numel.sum())
        return self._num_params

    def valid_bits(self) -> torch.Tensor:
        """int32 [ceil(P / 32)]: bit i & 31 of word i >> 5 is set iff element i belongs to a tensor
        (the eligibility mask of the top-k kernels; built once per layout)."""
        if self._vbits is None:
            v = self.seg_ids < self.nseg
            v = torch.cat([v, v.new_zeros((-self.P) % 32)]).view(-1, 32).long()
            w = (v << torch.arange(32, device=v.device)).sum(1)
            self._vbits = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()
        return self._vbits

    @classmethod
    def of(cls, layout, device) -> "LayoutMeta":
        off = torch.tensor([e.offset for e in layout.entries], dtype=torch.int64, device=device)
        numel = torch.tensor([e.numel for e in layout.entries], dtype=torch.int64, device=device)
        assert layout.padded_size % 8 == 0 and all(e.offset % 8 == 0 for e in layout.entries)
        return cls(layout.segment_ids(device), off, numel, len(layout.entries), layout.padded_size,
                   _num_params=layout.num_params)


@dataclass
class QuantPayload:
    kind: str  # "sq8" | "nnadq"
    codes: torch.Tensor  # uint8 [total bytes]
    row_off: torch.Tensor  # int64 [K + 1]
    seg_byte_off: torch.Tensor  # int64 [K, nseg]
    bits: torch.Tensor  # uint8 [K, nseg] (0: tensor not sent)
    lo: torch.Tensor  # fp32 [K, nseg]
    scale: torch.Tensor  # fp32 [K, nseg]
    meta: LayoutMeta
    row_off_host: list

    @property
    def K(self) -> int:
        return self.bits.shape[0]

    def row_bytes(self) -> list[int]:
        """Per client: code bytes + the metadata tensors of the tensors it sent."""
        per_seg = 9 if self.kind == "nnadq" else 4  # lo, scale, bit-width | the QSGD norm
        sent = (self.bits > 0).sum(1).cpu().tolist()
        off = self.row_off_host
        return [off[k + 1] - off[k] + per_seg * sent[k] for k in range(self.K)]

    def decode(self, out: torch.Tensor | None = None) -> torch.Tensor:
        K, P = self.K, self.meta.P
        if out is None:
            out = torch.empty((K, P), dtype=torch.float32, device=self.codes.device)
        assert out.shape == (K, P) and out.dtype == torch.float32 and out.stride(1) == 1
        if backend.get(out) is ref:
            out.copy_(_unpack_torch(self))
            return out
        from . import hip

        hip.quant_unpack(self, out)
        return out

    def accumulate(self, acc: torch.Tensor, w: torch.Tensor) -> None:
        """acc [P] fp64 += Σ_k w[k]·x̂_k (the server's FedAvg accumulation, fused)."""
        assert acc.dtype == torch.float64 and acc.shape == (self.meta.P,)
        w = w.to(acc.device, torch.float64).contiguous()
        if backend.get(acc) is ref:
            acc += (w[:, None] * _unpack_torch(self).double()).sum(0)
            return
        from . import hip

        hip.quant_unpack_acc(self, w, acc)


# ------------------------------------------------------------------ packing
def _segment_stats(x, meta: LayoutMeta):
    be = backend.get(x)
    if be is not ref:
        mn, mx = be.seg_minmax(x, meta.seg_ids, meta.nseg + 1)
        sq = be.seg_sq_sums(x, meta.seg_ids, meta.nseg + 1)
    else:
        K = x.shape[0]
        idx = meta.seg_ids.long().unsqueeze(0).expand(K, -1)
        mn = torch.full((K, meta.nseg + 1), float("inf"), device=x.device)
        mx = torch.full((K, meta.nseg + 1), float("-inf"), device=x.device)
        mn.scatter_reduce_(1, idx, x.float(), reduce="amin", include_self=True)
        mx.scatter_reduce_(1, idx, x.float(), reduce="amax", include_self=True)
        sq = torch.zeros((K, meta.nseg + 1), device=x.device)
        sq.index_add_(1, meta.seg_ids.long(), x.float() ** 2)
    return mn[:, : meta.nseg], mx[:, : meta.nseg], sq[:, : meta.nseg]


def _offsets(bits: torch.Tensor, meta: LayoutMeta):
    seg_bytes = (bits.long() * meta.seg_numel[None, :] + 7) // 8  # [K, nseg]
    seg_byte_off = torch.cumsum(seg_bytes, 1) - seg_bytes
    row_bytes = seg_bytes.sum(1)
    row_off = torch.zeros(bits.shape[0] + 1, dtype=torch.int64, device=bits.device)
    row_off[1:] = torch.cumsum(row_bytes, 0)
    return seg_byte_off.contiguous(), row_off


def _pack(kind: str, x: torch.Tensor, meta: LayoutMeta, bits, lo, scale, seeds) -> QuantPayload:
    seg_byte_off, row_off = _offsets(bits, meta)
    host = row_off.cpu().tolist()
    codes = torch.zeros(host[-1], dtype=torch.uint8, device=x.device)
    p = QuantPayload(kind, codes, row_off, seg_byte_off, bits.to(torch.uint8).contiguous(), lo.float().contiguous(),
                     scale.float().contiguous(), meta, host)
    if backend.get(x) is ref:
        _pack_torch(p, x, seeds)
    else:
        from . import hip

        hip.quant_pack(p, x, seeds)
    return p


def pack_stochastic(x: torch.Tensor, meta: LayoutMeta, seeds: list[int], seg_mask: torch.Tensor | None = None,
                    levels: int = 255) -> QuantPayload:
    """255-level QSGD stochastic quantisation of rows x [K, P] into an 8-bit payload."""
    from .quant import qsgd_range

    assert levels == 255, "the stochastic payload packs 8-bit codes"
    mn, mx, _ = _segment_stats(x, meta)
    lo, scale, _ = qsgd_range(mn, mx, levels)
    bits = torch.full_like(mn, 8, dtype=torch.uint8)
    if seg_mask is not None:
        bits = torch.where(seg_mask.to(bits.device), bits, torch.zeros_like(bits))
    return _pack("sq8", x, meta, bits, lo, scale, seeds)


def pack_nnadq(x: torch.Tensor, meta: LayoutMeta, weight: float, seg_mask: torch.Tensor | None = None) -> QuantPayload:
    """NNADQ: per-tensor adaptive bit-width (quant.nnadq_bits), round-to-nearest codes."""
    from .quant import nnadq_bits

    mn, mx, sq = _segment_stats(x, meta)
    rms = (sq / meta.seg_numel[None, :].float().clamp(min=1)).sqrt()
    b = nnadq_bits(mn, mx, rms, weight)
    levels = 2 ** b - 1
    lo = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
    scale = ((mx - mn) / levels).clamp(min=1e-30)
    scale = torch.where(torch.isfinite(scale), scale, torch.ones_like(scale))
    bits = b.to(torch.uint8)
    if seg_mask is not None:
        bits = torch.where(seg_mask.to(bits.device), bits, torch.zeros_like(bits))
    return _pack("nnadq", x, meta, bits, lo, scale, None)


# ------------------------------------------------------------------ CPU oracle
def _group_tables(p: QuantPayload):
    """Per flat 8-element group: its tensor, element index and valid count."""
    meta = p.meta
    t = torch.arange(meta.P // 8, device=p.codes.device)
    s = meta.seg_ids.long()[t * 8]
    real = s < meta.nseg
    t, s = t[real], s[real]
    j0 = t * 8 - meta.seg_off[s]
    n = torch.clamp(meta.seg_numel[s] - j0, max=8)
    return t, s, j0, n


def _codes_torch(p: QuantPayload, x: torch.Tensor, seeds) -> torch.Tensor:
    K = x.shape[0]
    sid = p.meta.seg_ids.long().clamp(max=p.meta.nseg - 1)
    lo, sc = p.lo[:, sid], p.scale[:, sid]
    # QSGD codes stop at 2s = 2^b − 2 (255 signed levels); NNADQ uses all 2^b levels
    top = (2 ** p.bits.long()[:, sid] - (2 if p.kind == "sq8" else 1)).float()
    r = (x.float() - lo) / sc
    if p.kind == "sq8":
        q = torch.floor(r + uniform_rows(seeds, x.shape[1], x.device))
    else:
        q = torch.round(r)
    q = torch.minimum(q.clamp(min=0), top)
    return q.long().view(K, -1)


def _pack_torch(p: QuantPayload, x: torch.Tensor, seeds) -> None:
    q = _codes_torch(p, x, seeds)  # [K, P]
    t, s, j0, n = _group_tables(p)
    K = x.shape[0]
    lane = torch.arange(8, device=x.device)
    for k in range(K):
        b = p.bits[k].long()[s]  # [G]
        sel = b > 0
        tt, ss, jj, nn, bb = t[sel], s[sel], j0[sel], n[sel], b[sel]
        codes = q[k].view(-1, 8)[tt]  # [G, 8]
        codes = torch.where(lane[None, :] < nn[:, None], codes, torch.zeros_like(codes))
        word = (codes << (lane[None, :] * bb[:, None])).sum(1)  # disjoint bit fields
        base = p.row_off[k] + p.seg_byte_off[k, ss] + (jj // 8) * bb
        nbytes = (nn * bb + 7) // 8
        for i in range(8):
            m = i < nbytes
            p.codes[base[m] + i] = ((word[m] >> (8 * i)) & 0xFF).to(torch.uint8)


def _unpack_torch(p: QuantPayload) -> torch.Tensor:
    K, P = p.K, p.meta.P
    out = torch.zeros((K, P), dtype=torch.float32, device=p.codes.device)
    t, s, j0, n = _group_tables(p)
    lane = torch.arange(8, device=p.codes.device)
    for k in range(K):
        b = p.bits[k].long()[s]
        sel = b > 0
        tt, ss, jj, nn, bb = t[sel], s[sel], j0[sel], n[sel], b[sel]
        base = p.row_off[k] + p.seg_byte_off[k, ss] + (jj // 8) * bb
        nbytes = (nn * bb + 7) // 8
        word = torch.zeros_like(base)
        for i in range(8):
            m = i < nbytes
            word[m] |= p.codes[base[m] + i].long() << (8 * i)
        q = (word[:, None] >> (lane[None, :] * bb[:, None])) & ((1 << bb[:, None]) - 1)
        v = p.lo[k, ss][:, None] + q.float() * p.scale[k, ss][:, None]
        v = torch.where(lane[None, :] < nn[:, None], v, torch.zeros_like(v))
        out[k].view(-1, 8)[tt] = v
    return out


# ------------------------------------------------------------------ top-k sparse payloads
@dataclass
class SparsePayload:
    """Top-k upload of K clients: per row the k selected flat (padded-layout) indices, ascending,
    and the values at them, verbatim. Selection rule (CPU oracle below ≡ csrc/topk.hip): the key of
    element i is bits(u[i]) & 0x7fffffff; inter-tensor padding is never eligible; the k eligible
    elements with the largest keys are selected, ties at the threshold key go to the lower index."""

    idx: torch.Tensor  # int32 [K, k]
    val: torch.Tensor  # fp32 [K, k]
    meta: LayoutMeta
    k: int

    @property
    def K(self) -> int:
        return self.idx.shape[0]

    def row_bytes(self) -> list[int]:
        """Per client: its int32 indices + its fp32 values."""
        per = self.idx[0].numel() * self.idx.element_size() + self.val[0].numel() * self.val.element_size()
        return [per] * self.K

    def decode(self, out: torch.Tensor | None = None) -> torch.Tensor:
        K, P = self.K, self.meta.P
        if out is None:
            out = torch.empty((K, P), dtype=torch.float32, device=self.val.device)
        assert out.shape == (K, P) and out.dtype == torch.float32 and out.stride(1) == 1
        if backend.get(out) is ref:
            out.zero_()
            out.scatter_(1, self.idx.long(), self.val)
            return out
        from . import hip

        hip.topk_decode(self, out)
        return out

    def accumulate(self, acc: torch.Tensor, w: torch.Tensor) -> None:
        """acc [P] fp64 += Σ_k w[k]·S(u_k), clients added in row order (work ∝ K·k, not K·P)."""
        assert acc.dtype == torch.float64 and acc.shape == (self.meta.P,)
        w = w.to(acc.device, torch.float64).contiguous()
        if backend.get(acc) is ref:
            acc += (w[:, None] * self.decode().double()).sum(0)
            return
        from . import hip

        hip.topk_accumulate(self, w, acc)


def _check_topk(u: torch.Tensor, meta: LayoutMeta, k: int) -> None:
    assert u.dim() == 2 and u.shape[1] == meta.P and u.dtype == torch.float32 and u.stride(1) == 1
    assert meta.P < 2 ** 31, "top-k indices are int32"
    assert 1 <= k <= meta.num_params, f"k = {k} outside [1, num_params]"


def _select_torch(u: torch.Tensor, meta: LayoutMeta, k: int) -> SparsePayload:
    """The oracle: torch.topk over the int64 composite (key << 32) | (0xffffffff − i), whose values
    are unique (no dependence on torch's tie order); ineligible elements get −1."""
    P = meta.P
    key = u.contiguous().view(torch.int32).long() & 0x7FFFFFFF
    i = torch.arange(P, device=u.device)
    comp = (key << 32) | (0xFFFFFFFF - i)[None, :]
    comp = torch.where((meta.seg_ids < meta.nseg)[None, :], comp, torch.full_like(comp, -1))
    idx = comp.topk(k, dim=1).indices.sort(dim=1).values
    return SparsePayload(idx.to(torch.int32), u.gather(1, idx), meta, k)


def pack_topk(u: torch.Tensor, meta: LayoutMeta, k: int) -> SparsePayload:
    """Top-k selection of rows u [K, P] (u is not modified)."""
    _check_topk(u, meta, k)
    if backend.get(u) is ref:
        return _select_torch(u, meta, k)
    from . import hip

    idx, val = hip.topk_pack(None, u, meta, k)
    return SparsePayload(idx, val, meta, k)


def pack_topk_ef(delta: torch.Tensor, err: torch.Tensor, meta: LayoutMeta, k: int) -> SparsePayload:
    """Error-feedback top-k: selects from u = delta + err and leaves err ← u − S(u) in place (u with
    the selected entries zeroed). delta [K, P] is only read; err [K, P] are the residual rows."""
    _check_topk(delta, meta, k)
    _check_topk(err, meta, k)
    assert err.shape == delta.shape and err.data_ptr() != delta.data_ptr()
    if backend.get(delta) is ref:
        err += delta
        p = _select_torch(err, meta, k)
        err.scatter_(1, p.idx.long(), 0.0)
        return p
    from . import hip

    idx, val = hip.topk_pack(delta, err, meta, k)
    return SparsePayload(idx, val, meta, k)


# ------------------------------------------------------------------ 1-bit rotated payloads (DRIVE / EDEN)
ROT_BLOCK = 4096  # 4⁶: the normalisation 1/√B = 2⁻⁶ is an exact scaling


@dataclass
class RotSignPayload:
    """1-bit upload of K clients (fed_drive, csrc/rotsign.hip): per row and per block of 4096 flat
    elements the sign bits of its randomised Hadamard rotation and one fp32 scale. Contract (CPU
    oracle below ≡ the kernels), block b = flat indices [4096 b, 4096 (b + 1)):
    - u_i reads as +0.0 at i ≥ P and at inter-tensor padding; z_i = u_i · d_i with d_i = −1 iff bit 31
      of mix32(i, seed_k) is set (`fl.uniform_rows`' hash of the flat index);
    - fp32 FWHT: stages h = 1, 2, …, 2048 in that order, (a, b) → (a + b, a − b) for the pairs
      (j, j + h) with j & h = 0, one rounding each; y = z′ · 2⁻⁶;
    - L1 = Σ|y_j|, L2 = Σ y_j² in fp64, each added as an adjacent-pair tree over j;
    - scale S = fp32(L2 / L1) ("unbiased", DRIVE: ⟨x̂, u⟩ = ‖u‖²) or fp32(L1 / 4096) ("mse": the
      projection onto the sign pattern, for error feedback); L1 = 0 gives S = 0;
    - bit j = sign bit of y_j, LSB-first (byte j >> 3, bit j & 7);
    - decode: t_j = ±S from the bits, the same FWHT, · 2⁻⁶, · d_i; 0.0 at padding.
    A non-finite element makes its block's scale, and so its decoded block, non-finite."""

    bits: torch.Tensor  # uint8 [K, nb · 512]
    scale: torch.Tensor  # fp32 [K, nb]
    seeds: list
    meta: LayoutMeta
    _seeds_dev: torch.Tensor | None = None

    @property
    def K(self) -> int:
        return self.bits.shape[0]

    @property
    def nb(self) -> int:
        return self.scale.shape[1]

    def row_bytes(self) -> list[int]:
        """Per client: its code bytes + its fp32 block scales (516 per block)."""
        per = self.bits[0].numel() * self.bits.element_size() + self.scale[0].numel() * self.scale.element_size()
        return [per] * self.K

    def seeds_dev(self) -> torch.Tensor:
        """int32 [K] on the payload's device (the kernels' copy of `seeds`)."""
        if self._seeds_dev is None:
            self._seeds_dev = _rot_seeds(self.seeds, self.bits.device)
        return self._seeds_dev

    def decode(self, out: torch.Tensor | None = None) -> torch.Tensor:
        K, P = self.K, self.meta.P
        if out is None:
            out = torch.empty((K, P), dtype=torch.float32, device=self.bits.device)
        assert out.shape == (K, P) and out.dtype == torch.float32 and out.stride(1) == 1
        if backend.get(out) is ref:
            out.copy_(_rot_decode_torch(self))
            return out
        from . import hip

        hip.rotsign_unpack(self, out)
        return out

    def accumulate(self, acc: torch.Tensor, w: torch.Tensor) -> None:
        """acc [P] fp64: acc[i] = acc[i] + (w[k] · x̂_k[i]) for k ascending, product and sum rounded
        separately; padding is not touched."""
        assert acc.dtype == torch.float64 and acc.shape == (self.meta.P,)
        w = w.to(acc.device, torch.float64).contiguous()
        assert w.numel() == self.K
        if backend.get(acc) is ref:
            valid = self.meta.seg_ids < self.meta.nseg
            x = _rot_decode_torch(self).double()[:, valid]
            a = acc[valid]
            for k in range(self.K):
                a = a + w[k] * x[k]
            acc[valid] = a
            return
        from . import hip

        hip.rotsign_accumulate(self, w, acc)


def _rot_seeds(seeds, device) -> torch.Tensor:
    return torch.tensor([s & 0xFFFFFFFF for s in seeds], dtype=torch.int64).to(torch.int32).to(device)


def _rot_diag(seeds, n: int, device) -> torch.Tensor:
    """[K, n] fp32 ±1: −1 where bit 31 of the hash of (flat index, row seed) is set."""
    idx = torch.arange(n, device=device, dtype=torch.int64)
    return torch.stack([1.0 - 2.0 * (_mix(idx, s & 0xFFFFFFFF) >> 31).float() for s in seeds])


def _rot_fwht(z: torch.Tensor) -> torch.Tensor:
    """The contract's transform of every length-4096 vector along the last axis (fp32)."""
    shape = z.shape
    h = 1
    while h < ROT_BLOCK:
        z = z.reshape(-1, ROT_BLOCK // (2 * h), 2, h)
        a, b = z[:, :, 0, :], z[:, :, 1, :]
        z = torch.stack((a + b, a - b), dim=2)
        h *= 2
    return z.reshape(shape) * 2.0 ** -6


def _rot_tree(v: torch.Tensor) -> torch.Tensor:
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _rot_blocks(u: torch.Tensor, meta: LayoutMeta) -> torch.Tensor:
    """[K, nb · 4096]: the rows with +0.0 at padding and beyond P."""
    K, P = u.shape
    nb = -(-P // ROT_BLOCK)
    z = torch.zeros((K, nb * ROT_BLOCK), dtype=torch.float32, device=u.device)
    z[:, :P] = torch.where((meta.seg_ids < meta.nseg)[None, :], u, torch.zeros((), device=u.device))
    return z


def _rot_pack_torch(u: torch.Tensor, meta: LayoutMeta, seeds, mse: bool) -> RotSignPayload:
    K = u.shape[0]
    z = _rot_blocks(u, meta)
    nb = z.shape[1] // ROT_BLOCK
    y = _rot_fwht((z * _rot_diag(seeds, z.shape[1], u.device)).view(K, nb, ROT_BLOCK))
    yd = y.double()
    L1, L2 = _rot_tree(yd.abs()), _rot_tree(yd * yd)
    if mse:
        S = (L1 / ROT_BLOCK).float()
    else:
        S = torch.where(L1 == 0, torch.zeros_like(L1), L2 / L1).float()
    neg = (y.contiguous().view(torch.int32) < 0).view(K, nb * ROT_BLOCK // 8, 8).long()
    bits = (neg << torch.arange(8, device=u.device)).sum(2).to(torch.uint8)
    return RotSignPayload(bits.contiguous(), S.contiguous(), list(seeds), meta)


def _rot_decode_torch(p: RotSignPayload) -> torch.Tensor:
    K, nb, P = p.K, p.nb, p.meta.P
    dev = p.bits.device
    neg = ((p.bits.long()[:, :, None] >> torch.arange(8, device=dev)) & 1).bool().view(K, nb, ROT_BLOCK)
    S = p.scale[:, :, None]
    x = _rot_fwht(torch.where(neg, -S, S)).view(K, nb * ROT_BLOCK) * _rot_diag(p.seeds, nb * ROT_BLOCK, dev)
    return torch.where((p.meta.seg_ids < p.meta.nseg)[None, :], x[:, :P], torch.zeros((), device=dev))


def _check_rot(u: torch.Tensor, meta: LayoutMeta, seeds) -> None:
    assert u.dim() == 2 and u.shape[1] == meta.P and u.dtype == torch.float32 and u.stride(1) == 1
    assert meta.P < 2 ** 31, "the diagonal hashes a 32-bit flat index"
    assert len(seeds) == u.shape[0], "one seed per client row"


def pack_rotsign(u: torch.Tensor, meta: LayoutMeta, seeds: list[int], scale: str = "unbiased") -> RotSignPayload:
    """1-bit rotated payload of rows u [K, P] (u is not modified). scale: "unbiased" | "mse"."""
    assert scale in ("unbiased", "mse"), scale
    _check_rot(u, meta, seeds)
    if backend.get(u) is ref:
        return _rot_pack_torch(u, meta, seeds, scale == "mse")
    from . import hip

    sd = _rot_seeds(seeds, u.device)
    bits, S = hip.rotsign_pack(u, None, meta, sd, scale == "mse")
    return RotSignPayload(bits, S, list(seeds), meta, sd)


def pack_rotsign_ef(delta: torch.Tensor, err: torch.Tensor, meta: LayoutMeta, seeds: list[int]) -> RotSignPayload:
    """Error-feedback form ("mse" scale): packs u = delta + err and leaves err ← u − x̂ in place (0 at
    padding). delta [K, P] is only read; err [K, P] are the residual rows."""
    _check_rot(delta, meta, seeds)
    _check_rot(err, meta, seeds)
    assert err.shape == delta.shape and err.data_ptr() != delta.data_ptr()
    if backend.get(delta) is ref:
        u = delta + err
        p = _rot_pack_torch(u, meta, seeds, True)
        err.copy_(torch.where((meta.seg_ids < meta.nseg)[None, :], u - _rot_decode_torch(p), torch.zeros(())))
        return p
    from . import hip

    sd = _rot_seeds(seeds, delta.device)
    bits, S = hip.rotsign_pack(delta, err, meta, sd, True)
    return RotSignPayload(bits, S, list(seeds), meta, sd)


# ------------------------------------------------------------------ masked uploads (secure aggregation)
@dataclass
class MaskedPayload:
    """The uploads of K clients after `ops.fl.secagg_mask_rows`: int32 [K, P] words of Z_{2^32} (the memory of
    the delta rows they replaced). `wire` holds each client's bytes: the masked vector plus the protocol's
    key and share traffic (utils/secagg_protocol.py)."""

    rows: torch.Tensor  # int32 [K, P], row stride >= P
    wire: list

    @property
    def K(self) -> int:
        return self.rows.shape[0]

    def row_bytes(self) -> list[int]:
        return [int(b) for b in self.wire]

    def decode(self, out: torch.Tensor | None = None) -> torch.Tensor:
        raise RuntimeError("a masked upload has no dense form: only the sum of a round's uploads can be unmasked")

    def accumulate(self, acc: torch.Tensor, w: torch.Tensor | None = None) -> None:
        """acc [P] int64 += Σ_k rows[k] (unweighted: a weight would have to be applied before masking)."""
        from .fl import ring_sum

        assert w is None, "masked uploads are added unweighted"
        ring_sum(self.rows, acc)
