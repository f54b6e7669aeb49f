"""What the ops of ops.functional hand each other work with: the form a BatchNorm output takes
(BNOut), the links between a conv and the BatchNorm around it, apply passes deferred to their
consumer (Deferral) and the record a tensor carries them in (Tags)."""

from __future__ import annotations

import dataclasses
import enum

import torch


class BNOut(enum.IntEnum):
    """What a BatchNorm writes, chosen by who reads it (Fn.batch_norm `planes`; fp32 native)."""

    FP32 = 0  # fp32 only
    BOTH = 1  # fp32 for fp32 readers + split planes for the conv(s) that read it
    PLANES = 2  # planes only: read by nothing but split-plane convs (a ResNet block's inner BN)
    CONV_DEFER = 3  # as PLANES, the apply deferred to the ONE 3x3 stride-1 conv that reads it (DeferredBN)
    RES_FOLD = 4  # (no ReLU) not written: the next BatchNorm folds it as its residual (DeferredRes)
    STEM_DEFER = 5  # CONV_DEFER + a second reader, the next BatchNorm's residual fold (DeferredStemBN)

    @property
    def applied_now(self) -> "BNOut":
        """The form taken when the deferral or fold cannot happen: one apply pass writes it."""
        now = {BNOut.CONV_DEFER: BNOut.PLANES, BNOut.RES_FOLD: BNOut.FP32, BNOut.STEM_DEFER: BNOut.BOTH}
        return now.get(self, self)

    @property
    def reads_planes(self) -> bool:
        """Whether any reader takes split planes."""
        return self not in (BNOut.FP32, BNOut.RES_FOLD)


class ResidualLink:
    """Hands a second gradient of a residual block's input to the block's first conv, whose
    dgrad adds it in its epilogue: autograd then never materialises `dX_conv + dX_other` with a
    separate add pass over the block input.
    - identity shortcut: the block's last BN (whose backward runs first) deposits dX_shortcut;
    - downsample shortcut: the shortcut conv (`donor`) deposits its dX. Autograd normally runs
      it before the main branch reaches the first conv; if not, the first conv marks
      `receiver_done` and the donor returns its dX to autograd as usual (same result).
      A 1x1 stride-s donor (fp32 native) deposits only the stride grid — the only pixels its dX
      is non-zero on — as a dense [K, B, ceil(H/s), ceil(W/s), C] tensor (`compact` = s): one
      stride-1 GEMM instead of s² parity launches (s² − 1 of them writing zeros), and the
      receiver's class-(0, 0) launch alone reads it (ops.hip.conv_dgrad acc_compact)."""

    __slots__ = ("grad", "receiver_done", "compact", "receiver_stride")

    def __init__(self):
        self.grad = None
        self.receiver_done = False
        self.compact = 0
        self.receiver_stride = 1  # stride of the receiving conv (set by its forward)


class MaskedGrad:
    """A gradient g = dy · relu' kept as its factors: `dy` [K, ..., C] fp32 and the 1-bit ReLU mask
    [K, rows, C / 8]. The identity shortcut of a ResNet block hands its gradient to the block's first
    conv this way (ResidualLink.grad): that conv's dgrad epilogue gates dy by the bits while it adds
    it (ops.hip.conv_dgrad acc_mask), so the BN backward never writes dy·relu' and nobody reads it
    back. `dense()` builds the tensor for any other consumer."""

    __slots__ = ("dy", "mask")

    def __init__(self, dy, mask):
        self.dy, self.mask = dy, mask

    def dense(self):
        K, C = self.dy.shape[0], self.dy.shape[-1]
        bits = torch.arange(8, device=self.mask.device, dtype=torch.uint8)
        keep = ((self.mask.view(K, -1, C // 8, 1) >> bits) & 1).reshape(K, -1, C).bool()
        return torch.where(keep, self.dy.reshape(K, -1, C), torch.zeros((), dtype=self.dy.dtype,
                                                                          device=self.dy.device)).view(self.dy.shape)


class BNStats:
    """Links a conv to the BatchNorm that consumes its output:
    - statistics: the fp32 conv epilogue writes per-32-row Σy / Σy² partials (of the first
      `valid[k]` samples' rows) and the BN consumes them instead of re-reading y in a statistics
      pass. `part` stays None when the producing conv could not provide them (CPU oracle, bf16
      kernels, LDS-DMA path);
    - `dy_planes_ok`: the conv runs its dgrad and wgrad on split planes (csrc/conv_pl.hip), so
      the BN backward writes only dX's planes (ops.hip.bn_bwd dx_planes=2), never the fp32 dX."""

    __slots__ = ("valid", "part", "dy_planes_ok", "wgrad_bn_bwd_ok")

    def __init__(self, valid=None):
        self.valid = valid
        self.part = None
        self.dy_planes_ok = False
        # the conv's weight gradient is its backward's only reader of dY and can apply the BN
        # backward in its fp32 dY loader (DeferredBNBwd f32)
        self.wgrad_bn_bwd_ok = False


# BN backward passes that used a dgrad's partials ("used"), whose consumer wrote none (a strided
# or absent conv: "none"), or whose dY was not that dgrad's output ("fallback"): tests, reports
bn_bwd_parts_count = {"used": 0, "none": 0, "fallback": 0}


class BNBwdLink:
    """Links a training BatchNorm's output to the stride-1 conv that consumes it: that conv's dgrad
    epilogue writes the BN backward's partial sums Σĝ, Σĝ·x̂ (ĝ = dY·relu') while it stores dX
    (= the BN's dY), so the BN backward skips its reduction pass over dY and x (ops.hip.conv_dgrad
    bnb=). The BN uses them only if the dY autograd hands it is that very dgrad output, unmodified
    (`key` = storage pointer + version): any other gradient summed in (a second consumer, a late
    residual donor) makes it fall back to its own pass."""

    __slots__ = ("x", "mask", "mean", "rstd", "valid", "part", "key")

    def __init__(self, x, mask, mean, rstd, valid):
        self.x, self.mask, self.mean, self.rstd, self.valid = x, mask, mean, rstd, valid
        self.part = self.key = None

    def args(self, part):
        return (part, self.x, self.mask, self.mean, self.rstd, self.valid, None)


# --------------------------------------------------------------------------- tensor tags
@dataclasses.dataclass(slots=True, eq=False)
class Tags:
    """What a producer tells a tensor's consumers, carried by the tensor object as its one
    attribute `_dls` (read with tags(), written with tag()). Autograd may rebuild a tensor on the
    way; it then arrives untagged. A name that is not a field raises AttributeError."""

    # its bf16 (hi, lo) split planes [K, 2, *shape[1:]] (ops.hip.planes_buffer, csrc/conv_pl.hip), produced with it
    planes: torch.Tensor | None = None
    # its fp32 bytes ARE those planes, or are unwritten: only a planes GEMM or a deferral's named reader may take it
    planes_only: bool = False
    bn_defer: DeferredBN | None = None  # a BatchNorm output whose apply is left to the conv that reads it
    res_fold: DeferredRes | None = None  # a BatchNorm output whose apply is left to the next BatchNorm
    bnb: BNBwdLink | None = None  # a BatchNorm output: the link its consuming conv's dgrad fills
    bn_bwd: DeferredBNBwd | None = None  # a BatchNorm input gradient whose apply is left to a weight gradient
    owned: bool = False  # freshly written, read by nothing else: a consumer may reuse it in place


class _Untagged(Tags):
    __slots__ = ()

    def __init__(self):
        for f in dataclasses.fields(Tags):
            object.__setattr__(self, f.name, f.default)

    def __setattr__(self, name, value):
        raise AttributeError("the untagged default is shared and read-only: write with tag()")


_UNTAGGED = _Untagged()


def tags(t) -> Tags:
    """`t`'s tag record; the shared read-only defaults for an untagged tensor (or None)."""
    return getattr(t, "_dls", _UNTAGGED)


def tag(t, record: Tags | None = None, **fields) -> Tags:
    """Sets `fields` in `t`'s record, created if it has none. `record`: `t` takes this record — two
    tensor objects over one buffer share one, so a change through either shows on both."""
    rec = t._dls = record or getattr(t, "_dls", None) or Tags()
    for name, value in fields.items():
        setattr(rec, name, value)
    return rec


def _require_fp32(t, who: str):
    if tags(t).planes_only:
        raise RuntimeError(f"{who}: a planes-only activation reached an op that reads fp32 values")


# --------------------------------------------------------------------------- deferred applies
class Deferral:
    """An apply pass left to its consumer. The consumer either does the work in a kernel of its own
    and calls `taken(key)`, or calls `materialize()`: the ordinary one-kernel pass (`_apply`) into
    the same buffers, with the same bits. `count`: the counter dict both bump (None: not counted)."""

    __slots__ = ("pending", "count")

    def __init__(self, count=None):
        self.pending = True
        self.count = count

    def taken(self, key: str):
        self.pending = False
        if self.count is not None:
            self.count[key] += 1

    def materialize(self):
        if self.pending:
            self._apply()
            self.taken("materialized")


class DeferredBN(Deferral):
    """A BatchNorm(+ReLU) output whose apply pass is deferred to its one consumer, a 3x3 stride-1
    conv that applies it while staging its input (ops.hip.conv_halo_bn_fwd, csrc/conv_halo.hip
    BNF): the normalised activation is never read back from HBM. The BN hands autograd the
    planes-only alias of `yp` (BNOut.CONV_DEFER); in training the fused conv also writes the
    planes and ReLU bits (its weight gradient and the BN backward read them). A consumer that
    cannot fuse — or anything that needs the values first — calls `materialize()`."""

    __slots__ = ("x", "coef", "relu", "valid_rows", "yp", "mask", "write_out")

    def __init__(self, x, coef, relu, valid_rows, yp, mask, write_out, count=None):
        super().__init__(count)
        self.x, self.coef, self.relu, self.valid_rows = x, coef, relu, valid_rows
        self.yp, self.mask, self.write_out = yp, mask, write_out

    def _apply(self):
        from . import hip  # (here and below: ops.hip needs the built extension, so not at import)
        hip.bn_apply_only(self.x, self.coef, self.valid_rows, self.relu, self.yp, self.mask)


# two-reader deferred BNs (DeferredStemBN): applies taken by the halo conv ("conv") or folded into
# the next BN's residual add ("res"), and forms written by a pass of their own ("materialized")
stem_defer_count = {"conv": 0, "res": 0, "materialized": 0}


class DeferredStemBN(DeferredBN):
    """A DeferredBN with a second reader: the next BatchNorm, which takes the output as its residual
    (BNOut.STEM_DEFER: the CIFAR ResNet stem BN, read by layer1.0.conv1 and, through the identity
    shortcut, by layer1.0.bn2). The conv side is DeferredBN's (`pending`, `materialize()`: planes +
    ReLU bits). The residual side folds the apply into the reading BN (hip.bn_fwd res_coef +
    res_relu: the fp32 bits this BN's own pass would have stored) or calls `materialize_f32()`, which
    writes the fp32 form into a tensor of its own. The two readers are independent and each form is
    written at most once. Autograd carries the planes-only alias: any other reader fails (_require_fp32)."""

    __slots__ = ("y32",)

    def __init__(self, x, coef, relu, valid_rows, yp, mask, write_out):
        super().__init__(x, coef, relu, valid_rows, yp, mask, write_out, stem_defer_count)
        self.y32 = None

    def materialize_f32(self):
        if self.y32 is None:
            from . import hip
            self.y32 = torch.empty(self.x.shape, dtype=self.x.dtype, device=self.x.device)
            hip.bn_apply_only(self.x, self.coef, self.valid_rows, self.relu, None, y=self.y32)
            self.count["materialized"] += 1
        return self.y32


# downsample BN applies folded into the next BN ("folded") or run as their own pass ("materialized")
res_fold_count = {"folded": 0, "materialized": 0}


class DeferredRes(Deferral):
    """A BatchNorm output without ReLU whose one reader is the next BatchNorm, as its residual — a
    ResNet downsample shortcut's BN (BNOut.RES_FOLD): the statistics and (scale, shift) are
    computed, the output is never written, and the reader folds the apply into its own
    (hip.bn_fwd res_coef: act(bn2(x) + scale·x_ds + shift), the bits of applying it first). The
    backward needs no output (no ReLU). Anything else that needs the values calls materialize()."""

    __slots__ = ("x", "coef", "valid_rows", "y")

    def __init__(self, x, coef, valid_rows, y):
        super().__init__(res_fold_count)
        self.x, self.coef, self.valid_rows, self.y = x, coef, valid_rows, y

    def _apply(self):
        from . import hip
        hip.bn_apply_only(self.x, self.coef, self.valid_rows, False, None, y=self.y)


# deferred BN backward applies (DeferredBNBwd) taken by a weight gradient's loader ("wgrad") or run
# as their own pass ("materialized"), by output: split planes / fp32. Tests, reports
bn_bwd_defer_count = {"wgrad": 0, "materialized": 0}
bn_bwd_f32_defer_count = {"wgrad": 0, "materialized": 0}


class DeferredBNBwd(Deferral):
    """A training BatchNorm's input gradient dX whose apply pass is deferred to the conv that
    produced the BN's input: the BN backward computed only its coefficients (a, d, e) and dγ / dβ,
    and that conv's weight gradient builds dX = a·(dy·relu') + e·x + d in its dY loader. Any other
    consumer calls `materialize()`. `out`, unwritten until one of them ran, is
    - split planes (OPTIONS.bn_bwd_in_wgrad): autograd carries their planes-only alias, and the
      conv's backward runs its halo weight gradient first, in dY mode 2 (csrc/conv_halo_wgrad.hip),
      which stores the planes for the dgrad on the way;
    - or fp32 (`f32`, OPTIONS.bn_bwd_in_wgrad_f32: that conv's backward is a weight gradient alone, the
      ResNet stem's, on the fp32 TN kernel, ops.hip.conv_wgrad bn_bwd=): autograd carries `out` itself,
      tagged unreadable (_require_fp32); the consumer that materialised it clears the mark."""

    __slots__ = ("dy", "x", "mask", "coef", "valid_rows", "out", "f32")

    def __init__(self, dy, x, mask, coef, valid_rows, out, f32=False):
        super().__init__(bn_bwd_f32_defer_count if f32 else bn_bwd_defer_count)
        self.dy, self.x, self.mask, self.coef, self.valid_rows = dy, x, mask, coef, valid_rows
        self.out, self.f32 = out, f32

    def _apply(self):
        from . import hip
        apply = hip.bn_bwd_apply_f32 if self.f32 else hip.bn_bwd_apply_planes
        apply(self.dy, self.x, self.mask, self.coef, self.valid_rows, self.out)

    def wgrad_args(self):
        args = (self.dy, self.x, self.mask, self.coef, self.valid_rows)
        return args if self.f32 else args + (self.out,)
