"""The Rényi-DP accountant of fed_dp_avg (`utils/privacy.py`) against mpmath at 50 digits and against
closed forms."""

import functools
import math

import mpmath as mp
import pytest

from distributed_learning_simulator_amd.utils import privacy

ORDERS = privacy.ORDERS
QS, ZS = (1e-3, 0.1, 0.5), (0.5, 1.1, 4.0)


@functools.lru_cache(maxsize=None)
def _mp_rdp(alpha: int, z: float, q: float) -> float:
    """log(Σ_k C(α, k)(1 − q)^{α−k} q^k exp((k² − k) / (2z²))) / (α − 1) at 50 digits."""
    with mp.workdps(50):
        zz, qq = mp.mpf(z), mp.mpf(q)
        a = mp.fsum(mp.binomial(alpha, k) * (1 - qq) ** (alpha - k) * qq ** k * mp.exp(mp.mpf(k * k - k) / (2 * zz * zz))
                    for k in range(alpha + 1))
        return float(mp.log(a) / (alpha - 1))


def test_orders_are_the_integers_2_to_256():
    assert ORDERS == tuple(range(2, 257))


@pytest.mark.parametrize("z", ZS)
def test_full_participation_is_the_gaussian_mechanism_and_q0_is_free(z):
    for a in ORDERS:
        assert privacy.rdp_sampled_gaussian(a, z, 1.0) == a / (2 * z * z) == privacy.rdp_gaussian(a, z)
        assert privacy.rdp_sampled_gaussian(a, z, 0.0) == 0.0
    # ... and q -> 1 approaches it
    assert privacy.rdp_sampled_gaussian(8, z, 1 - 1e-12) == pytest.approx(8 / (2 * z * z), rel=1e-9)


@pytest.mark.parametrize("z", ZS)
@pytest.mark.parametrize("q", QS)
def test_sampled_gaussian_agrees_with_mpmath(q, z):
    worst = 0.0
    for a in ORDERS:
        got, exp = privacy.rdp_sampled_gaussian(a, z, q), _mp_rdp(a, z, q)
        assert math.isfinite(got) and got > 0
        worst = max(worst, abs(got - exp) / exp)
    print("q", q, "z", z, "worst relative error", worst)
    assert worst <= 1e-9


def test_alpha_256_at_z_half_overflows_a_plain_sum_but_not_the_accountant():
    with pytest.raises(OverflowError):
        math.exp((256 * 256 - 256) / (2 * 0.5 * 0.5))
    got = privacy.rdp_sampled_gaussian(256, 0.5, 0.1)
    assert got == pytest.approx(_mp_rdp(256, 0.5, 0.1), rel=1e-9) and 400 < got < 512


def test_rdp_is_monotone_in_q_and_in_the_inverse_noise():
    qs = [0.0, 1e-4, 1e-3, 0.01, 0.1, 0.3, 0.5, 0.9, 1.0]
    zs = [8.0, 4.0, 2.0, 1.1, 0.8, 0.5]
    for a in (2, 3, 8, 32, 256):
        for z in ZS:
            vals = [privacy.rdp_sampled_gaussian(a, z, q) for q in qs]
            assert all(x < y for x, y in zip(vals, vals[1:])), (a, z, vals)
        for q in (1e-3, 0.1, 0.5, 1.0):
            vals = [privacy.rdp_sampled_gaussian(a, z, q) for z in zs]
            assert all(x < y for x, y in zip(vals, vals[1:])), (a, q, vals)


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        privacy.rdp_sampled_gaussian(1, 1.0, 0.5)
    with pytest.raises(ValueError):
        privacy.rdp_sampled_gaussian(2, 1.0, 1.5)
    with pytest.raises(ValueError):
        privacy.epsilon(1.0, 3, 0.0)


@pytest.mark.parametrize("z", [0.5, 1.1, 4.0])
@pytest.mark.parametrize("delta", [1e-5, 1e-8])
def test_epsilon_against_the_continuous_optimum_and_brute_force(z, delta):
    prev = 0.0
    for T in (1, 2, 10, 100, 1000):
        eps = privacy.epsilon(z, T, delta)
        # the minimum of T α / (2z²) + ln(1/δ) / (α − 1) over real α > 1
        cont = T / (2 * z * z) + math.sqrt(2 * T * math.log(1 / delta)) / z
        assert eps >= cont * (1 - 1e-12), (T, eps, cont)
        brute = min(T * a / (2 * z * z) + math.log(1 / delta) / (a - 1) for a in range(2, 257))
        assert eps == pytest.approx(brute, rel=1e-14)
        assert eps > prev
        prev = eps
    # the optimum lies inside the grid here: the integer grid costs little
    assert privacy.epsilon(1.1, 10, 1e-5) <= 1.05 * (10 / (2 * 1.21) + math.sqrt(20 * math.log(1e5)) / 1.1)


@pytest.mark.parametrize("q", [1e-3, 0.1, 0.5])
def test_amplified_epsilon_is_the_brute_force_minimum_and_below_the_unamplified(q):
    z, delta = 1.1, 1e-5
    prev = 0.0
    for T in (1, 10, 100):
        eps = privacy.epsilon(z, T, delta, q=q)
        brute = min(T * _mp_rdp(a, z, q) + math.log(1 / delta) / (a - 1) for a in ORDERS)
        assert eps == pytest.approx(brute, rel=1e-9)
        assert prev < eps < privacy.epsilon(z, T, delta)
        prev = eps


def test_no_noise_is_infinite_and_no_round_is_free():
    assert privacy.epsilon(0.0, 5, 1e-5) == math.inf and privacy.epsilon(0.0, 5, 1e-5, q=0.1) == math.inf
    assert privacy.rdp_sampled_gaussian(4, 0.0, 0.3) == math.inf
    assert privacy.epsilon(1.0, 0, 1e-5) == 0.0
    assert privacy.epsilon(1.0, 7, 1e-5, q=0.0) == pytest.approx(math.log(1e5) / 255)
