"""The GroupNorm kernels of csrc/groupnorm.hip against the float64 oracle of gn_common, at the
smallest shapes where each of their paths can go wrong (gn_common.SHAPES), plus what the contract
promises bitwise: skipped samples, placement independence, reproducibility, planes.
test_groupnorm_oracle.py shows that each tolerance is attainable in fp32.
"""

import pytest
import torch

import gn_common as gc
import rowwise_common as rc
from distributed_learning_simulator_amd.ops import functional as Fn
from distributed_learning_simulator_amd.ops import ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _poison_partials(hip, x):
    """NaN in the per-sample dγ / dβ rows the next gn_bwd(·, x, …) folds: every row it reads must
    have been written by that launch."""
    K, B, C = x.shape[0], x.shape[1], x.shape[-1]
    hip._tn_part(hip.gn_workspace_floats(K, B, C), x.device).fill_(float("nan"))


def _close(errs, tols, what):
    print(what, " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    for k, e in errs.items():
        assert e <= tols[k], f"{what}: {k} rel err {e:.3g} > {tols[k]}"


TOLS = {"y": rc.F32_TOL, "mean": rc.F32_TOL, "rstd": rc.F32_TOL, "dx": rc.F32_TOL_DX, "dgamma": rc.F32_TOL,
        "dbeta": rc.F32_TOL}


def _fwd_bwd(hip, x, gamma, beta, dy, res, G, relu, valid=None, tols=TOLS, what=""):
    """Forward and backward of one configuration against the oracle. The backward oracle is given
    the kernel's own mean / rstd and gate."""
    out = hip.gn_fwd(x, gamma, beta, G, valid, relu, res)
    y, mean, rstd = out
    y2, m2, r2 = gc.gn_fwd64(x, gamma, beta, G, relu, res, valid)
    errs = {"y": rc.rel_err(y, y2), "mean": rc.rel_err(mean, m2), "rstd": rc.rel_err(rstd, r2)}
    _poison_partials(hip, x)
    dx, dg, db, dres = hip.gn_bwd(dy, x, y, mean, rstd, gamma, G, valid, relu, res is not None)
    gate = (y > 0) if relu else None
    dx2, dg2, db2, dres2 = gc.gn_bwd64(dy, x, gate, mean, rstd, gamma, G, valid)
    errs.update(dx=rc.rel_err(dx, dx2), dgamma=rc.rel_err(dg, dg2), dbeta=rc.rel_err(db, db2))
    _close(errs, tols, what)
    if res is not None:
        assert torch.equal(dres.cpu().double(), dres2)  # (a select of dy: exact)
    else:
        assert dres is None
    return y, mean, rstd, dx, dg, db


@pytest.mark.parametrize("relu_res", [False, True], ids=["plain", "relu_res"])
@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.SHAPE_IDS)
def test_groupnorm_f32(hip, shape, relu_res):
    K, B, H, W, C, G, Kw = shape
    x, gamma, beta, dy, res = _dev(*gc.gn_inputs(K, B, H, W, C, Kw=Kw))
    _fwd_bwd(hip, x, gamma, beta, dy, res if relu_res else None, G, relu_res, what=f"gn {shape}")


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.SHAPE_IDS)
def test_groupnorm_planes_are_split_planes(hip, shape):
    """With planes: the same y / mean / rstd bits, and the planes are the split of y."""
    K, B, H, W, C, G, Kw = shape
    x, gamma, beta, _, res = _dev(*gc.gn_inputs(K, B, H, W, C, Kw=Kw))
    plain = hip.gn_fwd(x, gamma, beta, G, None, True, res)
    y, mean, rstd, yp = hip.gn_fwd(x, gamma, beta, G, None, True, res, planes=True)
    assert all(rc.bits_equal(a, b) for a, b in zip((y, mean, rstd), plain))
    assert yp.shape == (K, 2, B, H, W, C) and yp.dtype == BF16
    want = torch.empty_like(yp)  # (hip.split_planes needs 16-element rows: 5 x 5 x 6 is not)
    if (B * H * W * C) % 16 == 0:
        want = hip.split_planes(y)
    else:
        ref.split_rows(y.view(K, -1), want.view(K, 2, -1))
    assert rc.bits_equal(yp, want)


def test_offset_rows(hip):
    """x of mean 64, std 1 (gn_common.OFFSET_TOL, with the figures measured for it; a one-pass
    variance errs by about 1e-4 here)."""
    K, B, H, W, C, G = gc.OFFSET_SHAPE
    x, gamma, beta, dy, res = _dev(*gc.offset_inputs())
    _fwd_bwd(hip, x, gamma, beta, dy, None, G, False, tols=gc.OFFSET_TOL, what="gn offset")


def test_valid_skips_samples_bitwise(hip):
    """valid = [3, 1, 0] with NaN in the skipped samples: zeros there, everything finite, and
    y / dx / dγ / dβ bitwise those of separate launches on the truncated batches."""
    K, B, H, W, C, G = 3, 3, 8, 8, 64, 2
    x, gamma, beta, dy, res = gc.gn_inputs(K, B, H, W, C, seed=3)
    valid = torch.tensor([3, 1, 0], dtype=torch.int32)
    xn, rn, dyn = gc.poison_skipped(valid, x, res, dy)
    xn, rn, dyn, gamma, beta, vd = _dev(xn, rn, dyn, gamma, beta, valid)
    y, mean, rstd, dx, dg, db = _fwd_bwd(hip, xn, gamma, beta, dyn, rn, G, True, valid=vd, what="gn valid")
    dres = hip.gn_bwd(dyn, xn, y, mean, rstd, gamma, G, vd, True, True)[3]
    for t in (y, mean, rstd, dx, dg, db, dres):
        assert torch.isfinite(t).all()
    zero32 = torch.zeros((), device=DEV)
    for k, n in enumerate(valid.tolist()):
        for t in (y, dx, dres, mean, rstd):  # +0 bit patterns
            assert rc.bits_equal(t[k, n:], zero32.expand(t[k, n:].shape))
        if n == 0:
            assert rc.bits_equal(dg[k], zero32.expand(C)) and rc.bits_equal(db[k], zero32.expand(C))
            continue
        xk, rk, dyk = (t[k:k + 1, :n].contiguous() for t in (xn, rn, dyn))
        yk, mk, sk = hip.gn_fwd(xk, gamma[k:k + 1], beta[k:k + 1], G, None, True, rk)
        _poison_partials(hip, xk)
        dxk, dgk, dbk, _ = hip.gn_bwd(dyk, xk, yk, mk, sk, gamma[k:k + 1], G, None, True, True)
        assert rc.bits_equal(y[k:k + 1, :n], yk) and rc.bits_equal(dx[k:k + 1, :n], dxk)
        assert rc.bits_equal(mean[k:k + 1, :n], mk) and rc.bits_equal(rstd[k:k + 1, :n], sk)
        assert rc.bits_equal(dg[k:k + 1], dgk) and rc.bits_equal(db[k:k + 1], dbk)


def test_placement_independence_bitwise(hip):
    """One sample's y, mean, rstd and dx are the same bits at (k, b) = (0, 0) of a K = 1, B = 1
    launch and at (2, 1) of a K = 3, B = 2 launch."""
    H, W, C, G = 8, 8, 64, 2
    x, gamma, beta, dy, res = _dev(*gc.gn_inputs(3, 2, H, W, C, seed=7))
    y, mean, rstd = hip.gn_fwd(x, gamma, beta, G, None, True, res)
    dx = hip.gn_bwd(dy, x, y, mean, rstd, gamma, G, None, True, True)[0]
    x1, r1, dy1 = (t[2:3, 1:2].contiguous() for t in (x, res, dy))
    y1, m1, s1 = hip.gn_fwd(x1, gamma[2:3], beta[2:3], G, None, True, r1)
    dx1 = hip.gn_bwd(dy1, x1, y1, m1, s1, gamma[2:3], G, None, True, True)[0]
    assert rc.bits_equal(y[2:3, 1:2], y1) and rc.bits_equal(dx[2:3, 1:2], dx1)
    assert rc.bits_equal(mean[2:3, 1:2], m1) and rc.bits_equal(rstd[2:3, 1:2], s1)


def test_two_runs_are_bitwise_equal(hip):
    K, B, H, W, C, G = 2, 3, 16, 16, 128, 2
    x, gamma, beta, dy, res = _dev(*gc.gn_inputs(K, B, H, W, C, seed=8))
    runs = []
    for _ in range(2):
        y, mean, rstd = hip.gn_fwd(x, gamma, beta, G, None, True, res)
        _poison_partials(hip, x)
        runs.append((y, mean, rstd) + hip.gn_bwd(dy, x, y, mean, rstd, gamma, G, None, True, True))
    assert all(rc.bits_equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("shape", [(2, 3, 8, 8, 64, 2), (2, 2, 5, 5, 6, 3), (2, 3, 4, 4, 512, 32)],
                         ids=["base", "c6", "l4_g32"])
def test_groupnorm_bf16(hip, shape):
    """The bf16 instance against ops.ref on the upcast inputs (statistics and sums in fp32)."""
    K, B, H, W, C, G = shape
    x, gamma, beta, dy, res = _dev(*gc.gn_inputs(K, B, H, W, C, dtype=BF16))
    y, mean, rstd = hip.gn_fwd(x, gamma, beta, G, None, True, res)
    assert y.dtype == BF16 and mean.dtype == torch.float32
    y2, m2, r2 = ref.gn_fwd(x.float(), gamma.float(), beta.float(), G, None, True, res.float())
    rc.close(y, y2, rc.BF16_TOL, "y")
    rc.close(mean, m2, rc.BF16_TOL, "mean")
    rc.close(rstd, r2, rc.BF16_TOL, "rstd")
    dx, dg, db, dres = hip.gn_bwd(dy, x, y, mean, rstd, gamma, G, None, True, True)
    # (the reference takes the kernel's gate: bf16 rounding moves y across 0 now and then)
    dx2, dg2, db2, dres2 = ref.gn_bwd(dy.float(), x.float(), y.float(), m2, r2, gamma.float(), G, None, True, True)
    assert dx.dtype == BF16 and dg.dtype == torch.float32
    rc.close(dx, dx2, rc.BF16_TOL_DX, "dx")
    rc.close(dg, dg2, rc.BF16_TOL, "dgamma")
    rc.close(db, db2, rc.BF16_TOL, "dbeta")
    assert torch.equal(dres.float(), dres2)


def test_functional_group_norm_matches_cpu(hip):
    """Fn.group_norm on the GPU against the CPU path (ops.ref, which test_groupnorm_oracle.py ties to
    Fn.group_norm on the CPU): y, dx, what lands in ggamma / gbeta, and the residual's gradient,
    through autograd and through a ResidualLink. The CPU backward takes the GPU's ReLU gate. Bounds:
    both sides are within F32_TOL (dx: F32_TOL_DX) of float64, so twice that of each other."""
    K, B, H, W, C, G = 2, 3, 8, 8, 64, 2
    x, gamma, beta, dy, res = gc.gn_inputs(K, B, H, W, C, seed=4)
    valid = torch.tensor([3, 2], dtype=torch.int32)
    y2, m2, r2 = ref.gn_fwd(x, gamma, beta, G, valid, True, res)
    for link in (None, Fn.ResidualLink()):
        xa, ra = x.to(DEV).requires_grad_(), res.to(DEV).requires_grad_()
        token = torch.zeros(0, device=DEV, requires_grad=True)
        gg, gb = torch.full((K, C), 7.0, device=DEV), torch.full((K, C), 7.0, device=DEV)
        y = Fn.group_norm(xa, token, gamma.to(DEV), beta.to(DEV), gg, gb, G, valid.to(DEV), True, ra, link=link)
        y.backward(dy.to(DEV))
        dres = ra.grad if link is None else link.grad
        assert link is None or ra.grad is None
        dx2, dg2, db2, dres2 = ref.gn_bwd(dy, x, y.detach().cpu(), m2, r2, gamma, G, valid, True, True)
        rc.close(y, y2, 2 * rc.F32_TOL, "y")
        rc.close(xa.grad, dx2, 2 * rc.F32_TOL_DX, "dx")
        rc.close(gg, dg2, 2 * rc.F32_TOL, "ggamma")
        rc.close(gb, db2, 2 * rc.F32_TOL, "gbeta")
        assert torch.equal(dres.cpu(), dres2)
