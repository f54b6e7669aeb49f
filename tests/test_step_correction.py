"""The drift-corrected SGD step (ops.fl.sgd_step_corrected: FedProx / SCAFFOLD) on the CPU: `ops.ref`,
the oracle of the kernel and the CPU path, against the float64 step of rowwise_common fed with g'
formed in float64. The tolerance is the project's bound for optimiser steps
(rc.STEP_RTOL / rc.STEP_ATOL). (The kernel itself: test_step_correction_gpu.py.)
"""

import pytest
import torch

import rowwise_common as rc
from distributed_learning_simulator_amd.ops import fl, ref

P = 4096 + 80
MU = 0.1
MODES = ["mu", "corr", "both"]


def correction_inputs(P):
    """corr = 0.5·randn [3, P], anchor = randn [P] (shared by the GPU test)."""
    g = torch.Generator().manual_seed(31)
    return 0.5 * torch.randn(3, P, generator=g), torch.randn(P, generator=g)


def corrected_expected(setting, mode, P, mu=MU):
    """(θ_new, momentum_new) in float64: torch.optim.SGD's step on g' = g + corr + mu·(θ − anchor)."""
    theta, grad, mom, lr = rc.sgd_inputs(P)
    corr, anchor = correction_inputs(P)
    g = rc.d(grad)
    if mode in ("corr", "both"):
        g = g + rc.d(corr)
    if mode in ("mu", "both"):
        g = g + mu * (rc.d(theta) - rc.d(anchor)[None, :])
    return rc.sgd_step64(theta, g, mom, lr, rc.SGD_ACTIVE, rc.SGD_FIRST, *setting)


def mode_args(mode, corr, anchor, mu=MU):
    """(mu, anchor, corr) as the step takes them."""
    return (mu if mode != "corr" else 0.0, anchor if mode != "corr" else None, corr if mode != "mu" else None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("setting", rc.SGD_SETTINGS)
def test_sgd_step_corrected_ref_f32(setting, mode):
    momentum, dampening, nesterov, wd = setting
    theta0, grad0, mom0, lr = rc.sgd_inputs(P)
    theta, grad, mom = theta0.clone(), grad0.clone(), mom0.clone()
    corr0, anchor0 = correction_inputs(P)
    corr, anchor = corr0.clone(), anchor0.clone()
    mu, an, co = mode_args(mode, corr, anchor)
    fl.sgd_step_corrected(theta, grad, mom, lr, torch.tensor(rc.SGD_ACTIVE), torch.tensor(rc.SGD_FIRST), wd, momentum,
                          dampening, nesterov, mu, an, co)
    t2, m2 = corrected_expected(setting, mode, P)
    torch.testing.assert_close(theta.double(), t2, rtol=rc.STEP_RTOL, atol=rc.STEP_ATOL)
    torch.testing.assert_close(mom.double(), m2, rtol=rc.STEP_RTOL, atol=rc.STEP_ATOL)
    # the correction changed the step (the plain step's float64 result is far outside the bound)
    t_plain, _ = rc.sgd_expected(setting, P)
    assert (theta.double() - t_plain)[0].abs().max() > 1e-3
    # inactive row, read-only operands, momentum buffer without momentum
    assert rc.bits_equal(theta[1], theta0[1]) and rc.bits_equal(mom[1], mom0[1])
    assert rc.bits_equal(grad, grad0) and rc.bits_equal(corr, corr0) and rc.bits_equal(anchor, anchor0)
    if momentum == 0:
        assert rc.bits_equal(mom, mom0)


def test_sgd_step_corrected_ref_is_the_composition():
    """The oracle is literally: g' by separate fp32 operations, then ref.sgd_step."""
    momentum, dampening, nesterov, wd = rc.SGD_SETTINGS[2]
    theta0, grad, mom0, lr = rc.sgd_inputs(P)
    corr, anchor = correction_inputs(P)
    active, first = torch.tensor(rc.SGD_ACTIVE), torch.tensor(rc.SGD_FIRST)
    t1, m1 = theta0.clone(), mom0.clone()
    ref.sgd_step_corrected(t1, grad, m1, lr, active, wd, momentum, dampening, nesterov, first, MU, anchor, corr)
    t2, m2 = theta0.clone(), mom0.clone()
    g = grad + corr
    g = g + (t2 - anchor) * MU
    ref.sgd_step(t2, g, m2, lr, active, wd, momentum, dampening, nesterov, first)
    assert rc.bits_equal(t1, t2) and rc.bits_equal(m1, m2)
    # no correction at all: the plain step
    t3, m3 = theta0.clone(), mom0.clone()
    ref.sgd_step_corrected(t3, grad, m3, lr, active, wd, momentum, dampening, nesterov, first, 0.0, None, None)
    t4, m4 = theta0.clone(), mom0.clone()
    ref.sgd_step(t4, grad, m4, lr, active, wd, momentum, dampening, nesterov, first)
    assert rc.bits_equal(t3, t4) and rc.bits_equal(m3, m4)


def test_memory_plan_counts_extra_rows():
    """state_bytes_per_client: the three-argument value is unchanged, each extra row adds 4·P."""
    from distributed_learning_simulator_amd.engine.memory import state_bytes_per_client

    class L:
        padded_size = 1024

    base = state_bytes_per_client(L, torch.float32, "SGD")
    assert state_bytes_per_client(L, torch.float32, "SGD", extra_rows=0) == base
    assert state_bytes_per_client(L, torch.float32, "SGD", extra_rows=2) == base + 2 * 4 * 1024
