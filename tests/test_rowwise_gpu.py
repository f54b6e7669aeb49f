"""The row-wise kernels of csrc/norm.hip and csrc/elementwise.hip (LayerNorm, SGD / Adam steps,
weighted sums, block norms, segment min / max, column sums) against the float64 oracles of
rowwise_common, at the shapes where their launchers change path: every LayerNorm kernel instance,
both rows-per-wave walks, the second trip and ragged tail of every grid-stride loop, row strides
wider than the row, shared parameters, both reduction modes. test_rowwise_oracle.py shows that
each tolerance is attainable in fp32.
"""

import contextlib

import pytest
import torch

import rowwise_common as rc
from distributed_learning_simulator_amd.ops import fl, ref
from distributed_learning_simulator_amd.options import OPTIONS

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


@contextlib.contextmanager
def _atomics():
    """OPTIONS.deterministic = False (fp32 atomics instead of ordered folds) inside the block."""
    old = OPTIONS.deterministic
    OPTIONS.deterministic = False
    try:
        yield
    finally:
        OPTIONS.deterministic = old


def _dev(*ts):
    return [t.to(DEV) for t in ts]


# ------------------------------------------------------------------------ LayerNorm
def _ln_check_fwd(out, x, g, b):
    """y / mean / rstd of an fp32 launch against float64; returns the oracle's (mean, rstd)."""
    y2, m2, r2 = rc.ln_fwd64(x, g, b)
    errs = [rc.close(out[0], y2, rc.F32_TOL, "y"), rc.close(out[1], m2, rc.F32_TOL, "mean"),
            rc.close(out[2], r2, rc.F32_TOL, "rstd")]
    print("ln fwd", tuple(x.shape), "y/mean/rstd", " ".join(f"{e:.2g}" for e in errs))
    return m2, r2


def _ln_check_bwd(out, dy, x, m2, r2, g):
    """The kernel was fed its own mean / rstd; the oracle gets the oracle's."""
    dx2, dg2, db2 = rc.ln_bwd64(dy, x, m2, r2, g)
    errs = [rc.close(out[0], dx2, rc.F32_TOL_DX, "dx"), rc.close(out[1], dg2, rc.F32_TOL, "dgamma"),
            rc.close(out[2], db2, rc.F32_TOL, "dbeta")]
    print("ln bwd", tuple(x.shape), "dx/dgamma/dbeta", " ".join(f"{e:.2g}" for e in errs))


def _poison_ln_partials(hip, x):
    """NaN in the per-wave dγ / dβ partial rows of the next deterministic ln_bwd(·, x, …): a wave
    that has no rows must still write its (zero) row, the fold reads every one."""
    K, rows, C = x.shape
    hip._tn_part(hip._C.ln_workspace_floats(K, rows, C), x.device).fill_(float("nan"))


def _ln_f32(hip, K, rows, C, Kw=None, mean=0.0, planes=False):
    x, g, b, dy = _dev(*rc.ln_inputs(K, rows, C, Kw=Kw, mean=mean))
    out = hip.ln_fwd(x, g, b, planes=planes)
    m2, r2 = _ln_check_fwd(out, x, g, b)
    _poison_ln_partials(hip, x)
    _ln_check_bwd(hip.ln_bwd(dy, x, out[1], out[2], g), dy, x, m2, r2, g)
    return x, g, b, out


@pytest.mark.parametrize("C", [512, 1024])
def test_layernorm_pairs_kernels(hip, C):
    """ln_fwd_pairs_kernel<4> / <8>; 18 rows are not a multiple of the 4 rows of a workgroup. With
    planes: the same y bits, and the planes are split_planes(y). Backward NC = 8 / NC = 16."""
    x, g, b, plain = _ln_f32(hip, 2, 9, C)
    y, mean, rstd, yp = hip.ln_fwd(x, g, b, planes=True)
    assert rc.bits_equal(y, plain[0]) and rc.bits_equal(mean, plain[1]) and rc.bits_equal(rstd, plain[2])
    assert yp.shape == (2, 2, 9, C) and rc.bits_equal(yp, hip.split_planes(y))
    _ln_check_fwd((y, mean, rstd), x, g, b)


@pytest.mark.parametrize("C", [64, 65, 768, 1000])
def test_layernorm_generic_f32(hip, C):
    """ln_fwd_kernel with full and ragged column slots; C = 1000 is the NC = 16 backward."""
    x, g, b, out = _ln_f32(hip, 2, 37, C, planes=True)
    want = torch.empty_like(out[3])  # (hip.split_planes needs 16-element rows: 37 x 65 is not)
    ref.split_rows(out[0].view(2, -1), want.view(2, 2, -1))
    assert rc.bits_equal(out[3], want)


def _ln_bf16(hip, K, rows, C, mean=0.0):
    x, g, b, dy = _dev(*rc.ln_inputs(K, rows, C, mean=mean, dtype=BF16))
    y, mu, rs = hip.ln_fwd(x, g, b)
    y2, m2, r2 = ref.ln_fwd(x.float(), g.float(), b.float())
    assert y.dtype == BF16
    rc.close(y, y2, rc.BF16_TOL, "y")
    rc.close(mu, m2, rc.BF16_TOL, "mean")
    rc.close(rs, r2, rc.BF16_TOL, "rstd")
    dx, dg, db = hip.ln_bwd(dy, x, mu, rs, g)
    dx2, dg2, db2 = ref.ln_bwd(dy.float(), x.float(), m2, r2, g.float())
    rc.close(dx, dx2, rc.BF16_TOL_DX, "dx")
    rc.close(dg, dg2, rc.BF16_TOL, "dgamma")
    rc.close(db, db2, rc.BF16_TOL, "dbeta")


@pytest.mark.parametrize("C", [512, 1000])
def test_layernorm_generic_bf16(hip, C):
    _ln_bf16(hip, 2, 37, C)


def test_layernorm_bf16_offset_rows(hip):
    _ln_bf16(hip, 2, 37, 512, mean=4.0)


@pytest.mark.parametrize("rows", [4226, 4095])
def test_layernorm_rows_per_wave(hip, rows):
    """4226 rows: 128 rows per wave, 34 waves in 9 workgroups — the last wave with rows has 2, two
    waves have none and write zero partial rows. 4095 rows: 16 rows per wave, 64 workgroups."""
    _ln_f32(hip, 2, rows, 64)


def test_layernorm_shared_gamma(hip):
    """One γ / β row for K = 4 clients (Kw = 1), forward and backward."""
    _ln_f32(hip, 4, 9, 512, Kw=1)


@pytest.mark.parametrize("pad", [2, 1])
def test_layernorm_two_gamma_rows_strided(hip, pad):
    """Kw = 2 at K = 4 (γ row k // 2), the rows being views into a wider buffer: an even client
    stride keeps the pairs kernel, an odd one (8-B loads would be misaligned) the generic kernel."""
    K, rows, C = 4, 9, 512
    x, g, b, _ = _dev(*rc.ln_inputs(K, rows, C, Kw=2))
    gw = torch.full((2, C + pad), 7.0, device=DEV)
    bw = torch.full((2, C + pad), 7.0, device=DEV)
    gw[:, :C], bw[:, :C] = g, b
    gv, bv = gw[:, :C], bw[:, :C]
    assert gv.stride(0) == C + pad == bv.stride(0)
    _ln_check_fwd(hip.ln_fwd(x, gv, bv), x, g, b)


@pytest.mark.parametrize("C", [100, 512])
def test_layernorm_offset_rows(hip, C):
    """Rows of mean 64 and std 1. Σx²/C − μ² in fp32 loses (μ/σ)² = 4096 times the rounding of one
    term here (3e-4 in y); the kernels take Σ(x − μ)² in a second pass like ops.ref."""
    _ln_f32(hip, 2, 37, C, mean=64.0)


@pytest.mark.parametrize("rows,C", [(4226, 64), (37, 512)])
def test_layernorm_bwd_modes(hip, rows, C):
    """Deterministic mode: two calls agree bit for bit. Atomics mode: the same tolerances."""
    K = 2
    x, g, b, dy = _dev(*rc.ln_inputs(K, rows, C))
    y, mean, rstd = hip.ln_fwd(x, g, b)
    m2, r2 = _ln_check_fwd((y, mean, rstd), x, g, b)
    assert OPTIONS.deterministic
    _poison_ln_partials(hip, x)
    first = hip.ln_bwd(dy, x, mean, rstd, g)
    _poison_ln_partials(hip, x)
    second = hip.ln_bwd(dy, x, mean, rstd, g)
    for a, c in zip(first, second):
        assert rc.bits_equal(a, c)
    _ln_check_bwd(first, dy, x, m2, r2, g)
    with _atomics():
        out = hip.ln_bwd(dy, x, mean, rstd, g)
    assert OPTIONS.deterministic
    _ln_check_bwd(out, dy, x, m2, r2, g)


# ------------------------------------------------------------------ optimiser steps
def _step_close(out, exact):
    torch.testing.assert_close(out.cpu().double(), exact, rtol=rc.STEP_RTOL, atol=rc.STEP_ATOL)


@pytest.mark.parametrize("layout", ["split", "shadow_wide"])
@pytest.mark.parametrize("setting", rc.SGD_SETTINGS)
def test_sgd_step(hip, setting, layout):
    """P = 3·2^20 + 80: both float4s of a trip, a second trip and its ragged tail. `split`: rows at
    stride P with the weight planes; `shadow_wide`: rows of a [3, P + 16] buffer with a bf16 shadow,
    whose guard columns must come back untouched. Row 1 is inactive, row 2 on its first step."""
    momentum, dampening, nesterov, wd = setting
    theta0, grad0, mom0, lr = rc.sgd_inputs()
    P = rc.SGD_P
    active = torch.tensor(rc.SGD_ACTIVE, dtype=torch.bool, device=DEV)
    first = torch.tensor(rc.SGD_FIRST, dtype=torch.bool, device=DEV)
    t_exact, m_exact = rc.sgd_expected(setting)
    wides = []
    if layout == "split":
        theta, grad, mom = _dev(theta0, grad0, mom0)
        split = torch.full((3, 2, P), 3.0, dtype=BF16, device=DEV)
        hip.sgd_step(theta, grad, mom, lr.to(DEV), active, wd, momentum, dampening, nesterov, first, split=split)
        want = torch.full_like(split, 3.0)
        hip.split_rows(theta, want)
        want[1] = 3.0  # the inactive row keeps its planes
        assert rc.bits_equal(split, want)
    else:
        (tw, theta), (gw, grad), (mw, mom) = (rc.guarded(t.to(DEV)) for t in (theta0, grad0, mom0))
        sw, shadow = rc.guarded(theta0.to(DEV).to(BF16))
        shadow[1] = 5.0  # a stale shadow on the inactive row stays stale
        wides = [tw, gw, mw, sw]
        assert theta.stride(0) == P + 16 == shadow.stride(0)
        hip.sgd_step(theta, grad, mom, lr.to(DEV), active, wd, momentum, dampening, nesterov, first, shadow=shadow)
        want = theta.to(BF16)
        want[1] = 5.0
        assert rc.bits_equal(shadow, want)
        for w in wides:
            assert torch.all(w[:, P:] == 7.0)
        assert rc.bits_equal(grad, grad0.to(DEV))
    _step_close(theta, t_exact)
    _step_close(mom, m_exact)
    assert rc.bits_equal(theta[1].cpu(), theta0[1]) and rc.bits_equal(mom[1].cpu(), mom0[1])
    if momentum == 0:
        assert rc.bits_equal(mom.cpu(), mom0)


@pytest.mark.parametrize("setting", [rc.SGD_SETTINGS[0], rc.SGD_SETTINGS[2], rc.SGD_SETTINGS[3]])
def test_sgd_step_seg(hip, setting):
    """Spans of 1, 255, 256, 257, 513 and 1000 float4s (one workgroup of 256 threads x 2 float4 per
    trip each) with gaps between them: inside, the bits of sgd_step; outside, nothing changes."""
    momentum, dampening, nesterov, wd = setting
    counts, gap = [1, 255, 256, 257, 513, 1000], 3
    table, at = [], 2
    for n in counts:
        table.append((at, n))
        at += n + gap
    P = (4 * at + 15) // 16 * 16
    g = torch.Generator().manual_seed(21)
    theta, grad, mom = (torch.randn(3, P, generator=g).to(DEV) for _ in range(3))
    lr = torch.tensor([0.05, 0.3, 0.011], device=DEV)
    active = torch.tensor(rc.SGD_ACTIVE, dtype=torch.bool, device=DEV)
    first = torch.tensor(rc.SGD_FIRST, dtype=torch.bool, device=DEV)
    split = torch.full((3, 2, P), 3.0, dtype=BF16, device=DEV)
    inside = torch.zeros(P, dtype=torch.bool, device=DEV)
    for a, n in table:
        inside[4 * a:4 * (a + n)] = True
    t_all, m_all, s_all = theta.clone(), mom.clone(), split.clone()
    hip.sgd_step(t_all, grad, m_all, lr, active, wd, momentum, dampening, nesterov, first, split=s_all)
    t_seg, m_seg, s_seg = theta.clone(), mom.clone(), split.clone()
    hip.sgd_step_seg(t_seg, grad, m_seg, lr, active, wd, momentum, dampening, nesterov, first, s_seg,
                     torch.tensor(table, dtype=torch.int64, device=DEV))
    assert not rc.bits_equal(t_seg[0], theta[0])
    for got, stepped, before in ((t_seg, t_all, theta), (m_seg, m_all, mom), (s_seg, s_all, split)):
        assert rc.bits_equal(got[..., inside], stepped[..., inside])
        assert rc.bits_equal(got[..., ~inside], before[..., ~inside])


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_step(hip, wd, shadow):
    """adam_kernel against float64: P = 2·2^18 + 48 (two full trips of the stride loop and a ragged
    third), rows of a [4, P + 16] buffer, row 2 inactive, steps 1, 2, 10 and 1000, one lr per row."""
    theta0, grad0, m0, v0, lr = rc.adam_inputs()
    P = rc.ADAM_P
    (tw, theta), (gw, grad), (mw, m), (vw, v) = (rc.guarded(t.to(DEV)) for t in (theta0, grad0, m0, v0))
    wides = [tw, gw, mw, vw]
    sh = None
    if shadow:
        sw, sh = rc.guarded(theta0.to(DEV).to(BF16))
        sh[2] = 5.0
        wides.append(sw)
    b1, b2, eps = rc.ADAM_HYPER
    hip.adam_step(theta, grad, m, v, lr.to(DEV), torch.tensor(rc.ADAM_ACTIVE, dtype=torch.bool, device=DEV),
                  torch.tensor(rc.ADAM_STEP, device=DEV), b1, b2, eps, wd, shadow=sh)
    t2, m2, v2 = rc.adam_expected(wd)
    err = rc.update_err(theta, theta0, t2)
    print(f"adam_kernel update err per row (wd {wd:g}):", [f"{e:.3g}" for e in err.tolist()])
    for w in wides:
        assert torch.all(w[:, P:] == 7.0)
    for got, before in ((theta, theta0), (m, m0), (v, v0)):
        assert rc.bits_equal(got[2].cpu(), before[2])
    if shadow:
        want = theta.to(BF16)
        want[2] = 5.0
        assert rc.bits_equal(sh, want)
    _step_close(m, m2)
    _step_close(v, v2)
    _step_close(theta, t2)
    assert (err <= rc.ADAM_UPDATE_TOL).all(), err.tolist()


# ------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("K,P,pad", [(1, 4112, 16), (7, 4112, 16), (2, 8388608 + 48, 0)])
def test_weighted_sum_accumulates(hip, K, P, pad):
    """out += Σ_k w_k x_k into a non-zero fp64 accumulator, rows at stride P + pad; the last shape
    is 8192 workgroups x 256 threads x 4 plus 48: the grid-stride loop runs a second trip."""
    g = torch.Generator().manual_seed(K)
    xw, x = rc.guarded(torch.randn(K, P, generator=g).to(DEV), pad=pad) if pad else (None, torch.randn(
        K, P, generator=g).to(DEV))
    w = (torch.rand(K, generator=g) * 50).to(DEV)
    out0 = (torch.randn(P, generator=g, dtype=torch.float64) * 10).to(DEV)
    out = hip.weighted_sum(x, w, out0.clone())
    rc.close(out, rc.weighted_sum64(x, w.double(), out0), rc.SUM_TOL)
    assert rc.bits_equal(out, hip.weighted_sum(x, w, out0.clone()))
    assert not pad or torch.all(xw[:, P:] == 7.0)


def test_masked_weighted_sum_accumulates(hip):
    K, P = 5, 4112
    g = torch.Generator().manual_seed(31)
    x = torch.randn(K, P, generator=g).to(DEV)
    w = (torch.rand(K, generator=g) * 50).to(DEV)
    mask = torch.rand(K, P, generator=g) > 0.4
    mask[:, 5] = False  # masked in every row: num / den keep their bits
    mask[:, 4111] = False
    mask = mask.to(DEV)
    num0 = (torch.randn(P, generator=g, dtype=torch.float64) * 10).to(DEV)
    den0 = torch.rand(P, generator=g, dtype=torch.float64).to(DEV)
    num, den = hip.masked_weighted_sum(x, mask, w, num0.clone(), den0.clone())
    n2, d2 = rc.masked_weighted_sum64(x, mask, w.double(), num0, den0)
    rc.close(num, n2, rc.SUM_TOL)
    rc.close(den, d2, rc.SUM_TOL)
    for c in (5, 4111):
        assert rc.bits_equal(num[c], num0[c]) and rc.bits_equal(den[c], den0[c])
    again = hip.masked_weighted_sum(x, mask, w, num0.clone(), den0.clone())
    assert rc.bits_equal(num, again[0]) and rc.bits_equal(den, again[1])


def test_block_sq_norms(hip):
    """Σx² per (row, block) for runs that start and end inside a wave, on wave boundaries and across
    workgroup boundaries, with id −1 gaps (holding non-zero values) between some; P > 2^22, so the
    chunk loop runs a second trip. Each block within 1e-5 of its own float64 value: no block is
    longer than 65,536, 64 atomics, whose order changes the sum by far less."""
    ids, offsets, sizes = rc.block_layout()
    x = rc.block_inputs()
    exact = rc.block_sq64()
    xd, idd = x.to(DEV), ids.to(DEV)
    out = hip.block_sq_norms(xd, offsets.to(DEV), idd)
    assert out.shape == exact.shape and out.dtype == torch.float32
    e = rc.block_err(out, exact)
    print(f"block_sq_norms: worst block rel err {e:.3g}")
    assert e <= rc.F32_TOL
    # the same kernel through seg_sq_sums, rows of a wider buffer
    xw, xv = rc.guarded(xd)
    e = rc.block_err(hip.seg_sq_sums(xv, idd, sizes.numel()), exact)
    print(f"seg_sq_sums: worst block rel err {e:.3g}")
    assert e <= rc.F32_TOL
    # and against the CPU path, which adds a block's squares one after another in fp32: its own
    # rounding (rowwise_common.seq_sum_tol) on top of the kernel's bound
    cpu = fl.block_sq_norms(x, offsets, ids).double()
    assert ((out.cpu().double() - cpu).abs() <= (rc.F32_TOL + rc.seq_sum_tol(sizes)) * exact).all()


def test_seg_minmax(hip):
    """Exact min / max per (row, segment) through the integer-ordered atomics: one sign, both signs,
    single elements, ±0.0 (−0.0 orders as INT_MIN), denormals; segments inside a wave, across waves
    and across workgroups, rows of a wider buffer."""
    x, seg, nseg = rc.seg_inputs()
    xw, xv = rc.guarded(x.to(DEV))
    mn, mx = hip.seg_minmax(xv, seg.to(DEV), nseg)
    mn2, mx2 = rc.seg_minmax_exact(x, seg, nseg)
    bad = [(k, s, "min" if w == 0 else "max", got[k, s].item(), exp[k, s].item())
           for w, (got, exp) in enumerate(((mn.cpu(), mn2), (mx.cpu(), mx2)))
           for k in range(2) for s in range(nseg) if not got[k, s] == exp[k, s]]
    assert not bad, bad
    assert torch.all(xw[:, x.shape[1]:] == 7.0)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 7, 8195])
@pytest.mark.parametrize("C", [4, 10, 515, 1028, 2048])
def test_bias_grad_col_sum(hip, C, rows, dtype):
    """Column sums into a strided gradient view: the classifier's C = 10 (scalar form, 250 of 256
    threads) and AG-News' C = 4, C / V > 256 (a second column group: 515, 1028), one row, fewer rows
    than a workgroup covers, 8195 rows in 64 workgroups; ordered fold and atomics."""
    dy = rc.col_inputs(rows, C, dtype).to(DEV)
    exact = rc.col_sum64(dy)
    tol = rc.F32_TOL if dtype == torch.float32 else rc.BF16_TOL

    def run():
        gbuf = torch.full((2, C + 16), 7.0, device=DEV)
        gb = gbuf[:, 8:8 + C]
        hip.bias_grad(dy, gb)
        assert torch.all(gbuf[:, :8] == 7.0) and torch.all(gbuf[:, 8 + C:] == 7.0)
        rc.close(gb, exact, tol)
        return gb

    assert OPTIONS.deterministic
    assert rc.bits_equal(run(), run())
    with _atomics():
        run()
    assert OPTIONS.deterministic
