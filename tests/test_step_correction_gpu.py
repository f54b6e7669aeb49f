"""sgd_corr_kernel (csrc/elementwise.hip, ops.hip.sgd_step_corrected) on the GPU. Its contract is bit
equality with the two-pass form: g' = g + corr + mu·(θ − anchor) materialised by separate fp32
elementwise passes, then sgd_step. P = 3·2^20 + 80 as in test_rowwise_gpu.test_sgd_step (the kernel
has sgd_kernel's geometry): both float4s of a full trip of 1024 workgroups, and a ragged second trip.
"""

import pytest
import torch

import rowwise_common as rc
from test_step_correction import MODES, MU, corrected_expected, correction_inputs, mode_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
P = rc.SGD_P
GPU_SETTINGS = [rc.SGD_SETTINGS[0], rc.SGD_SETTINGS[2], rc.SGD_SETTINGS[3]]


def _flags():
    return (torch.tensor(rc.SGD_ACTIVE, dtype=torch.bool, device=DEV),
            torch.tensor(rc.SGD_FIRST, dtype=torch.bool, device=DEV))


def _two_pass_grad(theta, grad, corr, anchor, mode):
    """g' by separate torch passes, each rounding to fp32 once."""
    g = grad
    if mode != "mu":
        g = g + corr
    if mode != "corr":
        d = theta - anchor
        d = d * MU
        g = g + d
    return g


def _step_close(out, exact):
    torch.testing.assert_close(out.cpu().double(), exact, rtol=rc.STEP_RTOL, atol=rc.STEP_ATOL)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("setting", GPU_SETTINGS)
def test_corrected_step_has_the_bits_of_the_two_pass_form(hip, setting, mode):
    """θ, momentum, the split planes (first launch) and the bf16 shadow (second launch) against
    sgd_step on the materialised g'; and θ / momentum against the float64 step."""
    momentum, dampening, nesterov, wd = setting
    theta0, grad0, mom0, lr = (t.to(DEV) for t in rc.sgd_inputs())
    corr, anchor = (t.to(DEV) for t in correction_inputs(P))
    active, first = _flags()
    mu, an, co = mode_args(mode, corr, anchor)
    gp = _two_pass_grad(theta0, grad0, corr, anchor, mode)
    t_exact, m_exact = corrected_expected(setting, mode, P)
    for extra in ("split", "shadow"):
        def state():
            t, m = theta0.clone(), mom0.clone()
            if extra == "split":
                return t, m, {"split": torch.full((3, 2, P), 3.0, dtype=BF16, device=DEV)}
            return t, m, {"shadow": torch.full((3, P), 5.0, dtype=BF16, device=DEV)}

        t1, m1, kw1 = state()
        hip.sgd_step(t1, gp, m1, lr, active, wd, momentum, dampening, nesterov, first, **kw1)
        t2, m2, kw2 = state()
        hip.sgd_step_corrected(t2, grad0, m2, lr, active, wd, momentum, dampening, nesterov, first, mu, an, co, **kw2)
        assert rc.bits_equal(t2, t1), (extra, "theta")
        assert rc.bits_equal(m2, m1), (extra, "momentum")
        assert rc.bits_equal(kw2[extra], kw1[extra]), extra
        assert not rc.bits_equal(t2[0], theta0[0])
    _step_close(t2, t_exact)
    _step_close(m2, m_exact)
    if momentum == 0:
        assert rc.bits_equal(m2, mom0)


@pytest.mark.parametrize("extra", ["split", "shadow_wide"])
def test_corrected_step_layouts(hip, extra):
    """`split`: rows at stride P, the planes equal split_rows of the new θ, the inactive row keeps
    its planes. `shadow_wide`: θ / grad / momentum / shadow rows of [3, P + 16] buffers and corr rows
    of a [3, P + 48] buffer; every guard column comes back 7.0, the stale shadow of the inactive row
    stays. grad, corr and the anchor keep their bits, the inactive row is untouched."""
    momentum, dampening, nesterov, wd = rc.SGD_SETTINGS[2]
    theta0, grad0, mom0, lr = rc.sgd_inputs()
    corr0, anchor0 = correction_inputs(P)
    active, first = _flags()
    anchor = anchor0.to(DEV)
    if extra == "split":
        theta, grad, mom, corr = (t.to(DEV) for t in (theta0, grad0, mom0, corr0))
        split = torch.full((3, 2, P), 3.0, dtype=BF16, device=DEV)
        hip.sgd_step_corrected(theta, grad, mom, lr.to(DEV), active, wd, momentum, dampening, nesterov, first, MU,
                               anchor, corr, split=split)
        want = torch.full_like(split, 3.0)
        hip.split_rows(theta, want)
        want[1] = 3.0
        assert rc.bits_equal(split, want)
    else:
        (tw, theta), (gw, grad), (mw, mom) = (rc.guarded(t.to(DEV)) for t in (theta0, grad0, mom0))
        cw, corr = rc.guarded(corr0.to(DEV), pad=48)
        sw, shadow = rc.guarded(theta0.to(DEV).to(BF16))
        shadow[1] = 5.0
        assert theta.stride(0) == P + 16 and corr.stride(0) == P + 48
        hip.sgd_step_corrected(theta, grad, mom, lr.to(DEV), active, wd, momentum, dampening, nesterov, first, MU,
                               anchor, corr, shadow=shadow)
        want = theta.to(BF16)
        want[1] = 5.0
        assert rc.bits_equal(shadow, want)
        for w in (tw, gw, mw, cw, sw):
            assert torch.all(w[:, P:] == 7.0)
    t_exact, m_exact = corrected_expected(rc.SGD_SETTINGS[2], "both", P)
    _step_close(theta, t_exact)
    _step_close(mom, m_exact)
    assert rc.bits_equal(grad.cpu(), grad0) and rc.bits_equal(corr.cpu(), corr0)
    assert rc.bits_equal(anchor.cpu(), anchor0)
    assert rc.bits_equal(theta[1].cpu(), theta0[1]) and rc.bits_equal(mom[1].cpu(), mom0[1])


@pytest.mark.parametrize("setting", [rc.SGD_SETTINGS[0], rc.SGD_SETTINGS[2]])
def test_corrected_step_without_a_correction_is_sgd_step(hip, setting):
    """corr null and mu == 0: the bits of sgd_step (the anchor is not read)."""
    momentum, dampening, nesterov, wd = setting
    theta0, grad, mom0, lr = (t.to(DEV) for t in rc.sgd_inputs())
    active, first = _flags()
    t1, m1, s1 = theta0.clone(), mom0.clone(), torch.zeros((3, 2, P), dtype=BF16, device=DEV)
    hip.sgd_step(t1, grad, m1, lr, active, wd, momentum, dampening, nesterov, first, split=s1)
    t2, m2, s2 = theta0.clone(), mom0.clone(), torch.zeros((3, 2, P), dtype=BF16, device=DEV)
    hip.sgd_step_corrected(t2, grad, m2, lr, active, wd, momentum, dampening, nesterov, first, 0.0, None, None,
                           split=s2)
    assert rc.bits_equal(t2, t1) and rc.bits_equal(m2, m1) and rc.bits_equal(s2, s1)
