"""GroupNorm on the CPU: the float64 oracle of gn_common against torch's own group_norm + autograd,
and the fp32 CPU path (`ops.ref.gn_fwd` / `gn_bwd`) against the oracle at the tolerances the GPU
kernels are held to in test_groupnorm_gpu.py — which shows those tolerances are attainable in fp32.
"""

import pytest
import torch
import torch.nn.functional as F

import gn_common as gc
import rowwise_common as rc
from distributed_learning_simulator_amd.ops import functional as Fn
from distributed_learning_simulator_amd.ops import ref


def _nchw(t):
    K, B, H, W, C = t.shape
    return t.reshape(K * B, H, W, C).permute(0, 3, 1, 2)


def _nhwc(t, K):
    N, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(K, N // K, H, W, C)


@pytest.mark.parametrize("relu,with_res", [(False, False), (True, True), (True, False)])
@pytest.mark.parametrize("shape", [(2, 3, 8, 8, 64, 2), (2, 2, 5, 5, 6, 3), (2, 3, 8, 8, 64, 64)])
def test_oracle_matches_torch_group_norm_float64(shape, relu, with_res):
    """gn_fwd64 / gn_bwd64 == F.group_norm (+ residual, ReLU) and torch autograd, in float64."""
    K, B, H, W, C, G = shape
    x, gamma, beta, dy, res = (t.double() for t in gc.gn_inputs(K, B, H, W, C))
    y, mean, rstd = gc.gn_fwd64(x, gamma, beta, G, relu, res if with_res else None)
    outs, leaves = [], []
    for k in range(K):  # (torch's group_norm shares γ / β over the batch: one client at a time)
        xk, gk, bk, rk = (t[k:k + 1].clone().requires_grad_() for t in (x, gamma, beta, res))
        o = F.group_norm(_nchw(xk), G, gk[0], bk[0], eps=1e-5)
        if with_res:
            o = o + _nchw(rk)
        if relu:
            o = F.relu(o)
        o.backward(_nchw(dy[k:k + 1]))
        outs.append(_nhwc(o.detach(), 1))
        leaves.append((xk, gk, bk, rk))
    y_t = torch.cat(outs)
    assert rc.rel_err(y, y_t) <= 1e-12
    dx, dg, db, dres = gc.gn_bwd64(dy, x, (y > 0) if relu else None, mean, rstd, gamma, G)
    assert rc.rel_err(dx, torch.cat([l[0].grad for l in leaves])) <= 1e-12
    assert rc.rel_err(dg, torch.cat([l[1].grad for l in leaves])) <= 1e-12
    assert rc.rel_err(db, torch.cat([l[2].grad for l in leaves])) <= 1e-12
    if with_res:
        assert rc.rel_err(dres, torch.cat([l[3].grad for l in leaves])) <= 1e-12


def _check(impl_out, want, tols, what):
    errs = {}
    for name, got, exp in zip(("y", "mean", "rstd", "dx", "dgamma", "dbeta", "dres"), impl_out, want):
        if got is None:
            continue
        errs[name] = rc.rel_err(got, exp)
    print(what, " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e <= tols[name], f"{what}: {name} rel err {e:.3g} > {tols[name]}"
    return errs


F32_TOLS = {"y": rc.F32_TOL, "mean": rc.F32_TOL, "rstd": rc.F32_TOL, "dx": rc.F32_TOL_DX, "dgamma": rc.F32_TOL,
            "dbeta": rc.F32_TOL, "dres": 0.0}


def _ref_against_oracle(x, gamma, beta, dy, res, G, relu, with_res, tols, what, valid=None):
    r = res if with_res else None
    y, mean, rstd = ref.gn_fwd(x, gamma, beta, G, valid, relu, r)
    assert y.dtype == x.dtype and mean.dtype == torch.float32
    y2, m2, r2 = gc.gn_fwd64(x, gamma, beta, G, relu, r, valid)
    dx, dg, db, dres = ref.gn_bwd(dy, x, y, mean, rstd, gamma, G, valid, relu, with_res)
    # the oracle gets the implementation's own gate: a sign flip at |y| ~ 1e-7 is not an error
    gate = (y > 0) if relu else None
    want = (y2, m2, r2) + gc.gn_bwd64(dy, x, gate, m2, r2, gamma, G, valid)
    return _check((y, mean, rstd, dx, dg, db, dres), want, tols, what)


@pytest.mark.parametrize("relu,with_res", [(False, False), (True, True)])
@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.SHAPE_IDS)
def test_ref_matches_oracle(shape, relu, with_res):
    K, B, H, W, C, G, Kw = shape
    x, gamma, beta, dy, res = gc.gn_inputs(K, B, H, W, C, Kw=Kw)
    _ref_against_oracle(x, gamma, beta, dy, res, G, relu, with_res, F32_TOLS, f"ref {shape}")


def test_ref_offset_rows():
    """x of mean 64, std 1: the bounds of gn_common.OFFSET_TOL (their measured basis is there)."""
    K, B, H, W, C, G = gc.OFFSET_SHAPE
    x, gamma, beta, dy, res = gc.offset_inputs()
    tols = dict(gc.OFFSET_TOL, dres=0.0)
    _ref_against_oracle(x, gamma, beta, dy, res, G, False, False, tols, "ref offset")


def test_one_pass_variance_would_fail_the_offset_case():
    """The case exists to catch Σx²/n − mean²: in fp32 it misses the bound on this input."""
    K, B, H, W, C, G = gc.OFFSET_SHAPE
    x, gamma, beta, _, _ = gc.offset_inputs()
    xg = x.reshape(K, B, H * W, G, C // G)
    mean = xg.mean(dim=(2, 4))
    var = (xg * xg).mean(dim=(2, 4)) - mean * mean
    rstd = torch.rsqrt(var.clamp_min(0) + 1e-5)
    _, _, r2 = gc.gn_fwd64(x, gamma, beta, G)
    assert rc.rel_err(rstd, r2) > gc.OFFSET_TOL["rstd"]


def test_ref_valid_skips_samples():
    """valid = [3, 1, 0] with NaN in the skipped samples' x, residual and dy: finite outputs, zeros
    in the skipped samples, dγ / dβ of the truncated batch."""
    K, B, H, W, C, G = 3, 3, 8, 8, 64, 2
    x, gamma, beta, dy, res = gc.gn_inputs(K, B, H, W, C, seed=3)
    valid = torch.tensor([3, 1, 0], dtype=torch.int32)
    xn, rn, dyn = gc.poison_skipped(valid, x, res, dy)
    y, mean, rstd = ref.gn_fwd(xn, gamma, beta, G, valid, True, rn)
    dx, dg, db, dres = ref.gn_bwd(dyn, xn, y, mean, rstd, gamma, G, valid, True, True)
    for t in (y, mean, rstd, dx, dg, db, dres):
        assert torch.isfinite(t).all()
    for k, n in enumerate(valid.tolist()):
        for t in (y, dx, dres, mean, rstd):
            assert not t[k, n:].any()
        if n == 0:
            assert not dg[k].any() and not db[k].any()
            continue
        yk, mk, rk = ref.gn_fwd(x[k:k + 1, :n], gamma[k:k + 1], beta[k:k + 1], G, None, True, res[k:k + 1, :n])
        dxk, dgk, dbk, _ = ref.gn_bwd(dy[k:k + 1, :n], x[k:k + 1, :n], yk, mk, rk, gamma[k:k + 1], G, None, True, True)
        assert rc.rel_err(y[k:k + 1, :n], yk) <= 1e-6 and rc.rel_err(dx[k:k + 1, :n], dxk) <= 1e-6
        assert rc.rel_err(dg[k:k + 1], dgk) <= 1e-6 and rc.rel_err(db[k:k + 1], dbk) <= 1e-6
    _ref_against_oracle(xn, gamma, beta, dyn, rn, G, True, True, F32_TOLS, "ref valid", valid=valid)


def test_functional_group_norm_cpu():
    """Fn.group_norm under autograd: dγ / dβ land in ggamma / gbeta, the residual's gradient comes
    back through autograd, or through a ResidualLink with the same values; planes-only inputs are
    refused."""
    K, B, H, W, C, G = 2, 3, 8, 8, 64, 2
    x, gamma, beta, dy, res = gc.gn_inputs(K, B, H, W, C, seed=4)
    valid = torch.tensor([3, 2], dtype=torch.int32)
    token = torch.zeros(0, requires_grad=True)
    xa, ra = x.clone().requires_grad_(), res.clone().requires_grad_()
    gg, gb = torch.full((K, C), 7.0), torch.full((K, C), 7.0)
    y = Fn.group_norm(xa, token, gamma, beta, gg, gb, G, valid, True, ra)
    y.backward(dy)
    y2, mean, rstd = ref.gn_fwd(x, gamma, beta, G, valid, True, res)
    dx, dgam, dbet, dres = ref.gn_bwd(dy, x, y2, mean, rstd, gamma, G, valid, True, True)
    assert torch.equal(y.detach(), y2) and torch.equal(xa.grad, dx) and torch.equal(ra.grad, dres)
    assert torch.equal(gg, dgam) and torch.equal(gb, dbet)
    link = Fn.ResidualLink()
    xb, rb = x.clone().requires_grad_(), res.clone().requires_grad_()
    Fn.group_norm(xb, token, gamma, beta, gg, gb, G, valid, True, rb, link=link).backward(dy)
    assert rb.grad is None and torch.equal(link.grad, dres) and torch.equal(xb.grad, dx)
    only = x.clone()
    Fn.tag(only, planes_only=True)
    with pytest.raises(RuntimeError, match="planes-only"):
        Fn.group_norm(only, token, gamma, beta, gg, gb, G)
