"""Every tolerance of tests/test_rowwise_gpu.py is attainable in fp32: `ops.ref`, the CPU path, run
in fp32 on the same input classes stays inside it against the float64 oracles of rowwise_common.
(No GPU: the kernels themselves are compared in test_rowwise_gpu.py.)
"""

import pytest
import torch

import rowwise_common as rc
from distributed_learning_simulator_amd.ops import fl, ref


@pytest.mark.parametrize("K,rows,C,Kw,mean", [
    (2, 9, 512, None, 0.0), (2, 9, 1024, None, 0.0), (2, 37, 64, None, 0.0), (2, 37, 65, None, 0.0),
    (2, 37, 768, None, 0.0), (2, 37, 1000, None, 0.0), (2, 4226, 64, None, 0.0), (2, 4095, 64, None, 0.0),
    (4, 9, 512, 1, 0.0), (4, 9, 512, 2, 0.0),
    # offset rows: Σx²/C − μ² in fp32 is off by 3e-4 here, the two-pass reference by 2e-6
    (2, 37, 100, None, 64.0), (2, 37, 512, None, 64.0), (2, 37, 1024, None, 64.0),
])
def test_layernorm_ref_f32(K, rows, C, Kw, mean):
    x, g, b, dy = rc.ln_inputs(K, rows, C, Kw=Kw, mean=mean)
    y, mu, rs = ref.ln_fwd(x, g, b)
    y2, m2, r2 = rc.ln_fwd64(x, g, b)
    assert y.dtype == torch.float32
    errs = [rc.close(y, y2, rc.F32_TOL, "y"), rc.close(mu, m2, rc.F32_TOL, "mean"),
            rc.close(rs, r2, rc.F32_TOL, "rstd")]
    dx, dg, db = ref.ln_bwd(dy, x, mu, rs, g)
    dx2, dg2, db2 = rc.ln_bwd64(dy, x, m2, r2, g)
    errs += [rc.close(dx, dx2, rc.F32_TOL_DX, "dx"), rc.close(dg, dg2, rc.F32_TOL, "dgamma"),
             rc.close(db, db2, rc.F32_TOL, "dbeta")]
    print("ln ref fp32", (K, rows, C, Kw, mean), " ".join(f"{e:.2g}" for e in errs))


@pytest.mark.parametrize("setting", rc.SGD_SETTINGS)
def test_sgd_ref_f32(setting):
    P = 4096 + 80
    theta, grad, mom, lr = (t.clone() for t in rc.sgd_inputs(P))
    momentum, dampening, nesterov, wd = setting
    ref.sgd_step(theta, grad, mom, lr, torch.tensor(rc.SGD_ACTIVE), wd, momentum, dampening, nesterov,
                 torch.tensor(rc.SGD_FIRST))
    t2, m2 = rc.sgd_expected(setting, P)
    torch.testing.assert_close(theta.double(), t2, rtol=rc.STEP_RTOL, atol=rc.STEP_ATOL)
    torch.testing.assert_close(mom.double(), m2, rtol=rc.STEP_RTOL, atol=rc.STEP_ATOL)


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_ref_f32(wd):
    """Also the measurement behind rowwise_common.ADAM_REF_ERR (printed; the bound is four times it)."""
    theta0 = rc.adam_inputs()[0]
    theta, grad, m, v, lr = (t.clone() for t in rc.adam_inputs())
    b1, b2, eps = rc.ADAM_HYPER
    ref.adam_step(theta, grad, m, v, lr, torch.tensor(rc.ADAM_ACTIVE), torch.tensor(rc.ADAM_STEP), b1, b2, eps, wd)
    t2, m2, v2 = rc.adam_expected(wd)
    for out, exp in ((theta, t2), (m, m2), (v, v2)):
        torch.testing.assert_close(out.double(), exp, rtol=rc.STEP_RTOL, atol=rc.STEP_ATOL)
    err = rc.update_err(theta, theta0, t2)
    print("adam ref fp32 update err per row (wd %g):" % wd, [f"{e:.3g}" for e in err.tolist()])
    for k, t in enumerate(rc.ADAM_STEP):
        if rc.ADAM_ACTIVE[k]:
            # the recorded figure is what this reference gives: the bound is 4x a real number
            assert err[k].item() <= 1.5 * rc.ADAM_REF_ERR < rc.ADAM_UPDATE_TOL, (t, err[k].item())
        else:
            assert err[k].item() == 0.0


@pytest.mark.parametrize("K", [1, 7])
def test_weighted_sums_ref(K):
    P = 4112
    g = torch.Generator().manual_seed(K)
    x, w = torch.randn(K, P, generator=g), torch.rand(K, generator=g) * 50
    out0 = torch.randn(P, generator=g, dtype=torch.float64) * 10
    rc.close(ref.weighted_sum(x, w, out0.clone()), rc.weighted_sum64(x, w, out0), rc.SUM_TOL)
    mask = torch.rand(K, P, generator=g) > 0.4
    mask[:, 5] = False
    n0, d0 = out0.clone(), torch.rand(P, generator=g, dtype=torch.float64)
    n, dn = ref.masked_weighted_sum(x, mask, w, n0.clone(), d0.clone())
    n2, d2 = rc.masked_weighted_sum64(x, mask, w, n0, d0)
    rc.close(n, n2, rc.SUM_TOL)
    rc.close(dn, d2, rc.SUM_TOL)
    assert n[5] == n0[5] and dn[5] == d0[5]


def test_block_sq_norms_ref_f32():
    ids, offsets, sizes = rc.block_layout()
    assert ids.numel() > 4194304 and ids.numel() % 16 == 0 and int(sizes.max()) == 65536
    assert sorted(set(sizes.tolist())) == [16, 32, 1008, 1024, 1040, 4800, 65536]
    x, exact = rc.block_inputs(), rc.block_sq64()
    # 1e-5 per block is attainable in fp32: torch.sum adds the squares pairwise (measured 1.5e-7)
    tree = torch.stack([(x[:, a:a + n] ** 2).sum(1) for a, n in zip(rc.block_starts(), sizes.tolist())], dim=1)
    assert tree.dtype == torch.float32
    e = rc.block_err(tree, exact)
    print(f"block Σx², fp32 pairwise: worst block rel err {e:.3g}")
    assert e <= rc.F32_TOL
    # the CPU path adds each block one element after another (index_add_): 1.9e-5 at 65,536
    # elements, so it is held to the random-walk bound of that order, not to 1e-5
    out = fl.block_sq_norms(x, offsets, ids)
    assert out.dtype == torch.float32
    rel = (out.double() - exact).abs() / exact
    print(f"block Σx², CPU path: worst block rel err {rel.max().item():.3g}")
    assert (rel <= rc.seq_sum_tol(sizes)).all()


def test_seg_inputs_cover_every_class():
    x, seg, nseg = rc.seg_inputs()
    mn, mx = rc.seg_minmax_exact(x, seg, nseg)
    assert nseg >= 2 * len(rc.SEG_CLASSES) and x.shape == (2, 4112)
    neg_zero = (x == 0) & torch.signbit(x)
    all_nz = [bool(neg_zero[k, seg == s].all()) for k in range(2) for s in range(nseg)]
    assert any(all_nz)  # a segment holding only −0.0: its maximum is (−)0.0, not −inf
    assert ((x != 0) & (x.abs() < 1e-38)).any()  # denormals
    assert (mx < 0).any() and (mn > 0).any() and ((mn < 0) & (mx > 0)).any()
    assert ((mx == 0) & (mn < 0)).any()  # −0.0 is the maximum over negative values


@pytest.mark.parametrize("C", [4, 10, 515, 1028, 2048])
@pytest.mark.parametrize("rows", [1, 7, 8195])
def test_col_sum_ref_f32(rows, C):
    dy = rc.col_inputs(rows, C, torch.float32)
    rc.close(dy.sum(1), rc.col_sum64(dy), rc.F32_TOL)
