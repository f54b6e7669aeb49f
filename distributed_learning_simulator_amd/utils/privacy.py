"""Rényi-DP accountant for `fed_dp_avg` (host only; nothing beyond `math`).

The Gaussian mechanism with noise multiplier z (std = z · sensitivity) has Rényi divergence
α / (2z²) at order α (Mironov 2017). Run on a Poisson sample of rate q it has, at integer α ≥ 2
(Mironov, Talwar, Zhang 2019, "Rényi differential privacy of the sampled Gaussian mechanism"),

    A_α = Σ_{k=0..α} C(α, k) (1 − q)^{α−k} q^k · exp((k² − k) / (2z²)),    rdp(α) = log(A_α) / (α − 1).

RDP adds up over rounds, and T rounds convert to (ε, δ)-DP by

    ε = min_α [T · rdp(α) + ln(1/δ) / (α − 1)]

over the integer orders α = 2 … 256. Everything is evaluated in log space (`lgamma`, log-sum-exp):
at α = 256, z = 0.5 the largest term is exp(130560), far outside a double.

`epsilon(z, T, δ)` (q = 1) is the UNAMPLIFIED composition: it holds whatever the participation scheme
is. `epsilon(z, T, δ, q)` with q < 1 holds ONLY IF every round's clients were Poisson-sampled —
each client independently with probability q. The simulator draws a fixed-size subset instead, so
the figure it reports as `dp_epsilon_poisson` (q = m / worker_number) is indicative, not a guarantee.
"""

from __future__ import annotations

import math

ORDERS = tuple(range(2, 257))


def _log_add(a: float, b: float) -> float:
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


def rdp_gaussian(alpha: int, z: float) -> float:
    """Rényi divergence of order α of the Gaussian mechanism with noise multiplier z: α / (2z²)."""
    if z <= 0:
        return math.inf
    return alpha / (2.0 * z * z)


def rdp_sampled_gaussian(alpha: int, z: float, q: float) -> float:
    """RDP of order α (an integer ≥ 2) of the Poisson-subsampled Gaussian mechanism at sampling rate q
    (the formula of the module docstring, in log space). q = 0 gives 0, q = 1 gives α / (2z²)."""
    alpha = int(alpha)
    if alpha < 2:
        raise ValueError(f"integer orders alpha >= 2 only, got {alpha}")
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"the sampling rate must lie in [0, 1], got {q}")
    if q == 0.0:
        return 0.0
    if z <= 0:
        return math.inf
    if q == 1.0:
        return rdp_gaussian(alpha, z)
    # Σ_k C(α, k)(1 − q)^{α−k} q^k = 1 and the terms k = 0, 1 carry exp(0): A − 1 is the sum over k ≥ 2
    # with expm1 in place of exp — all terms positive, so log A keeps its relative accuracy where
    # A − 1 is tiny (small q) as well as where it overflows a double
    log_q, log_1q = math.log(q), math.log1p(-q)
    lg = math.lgamma
    log_excess = -math.inf  # log(A − 1)
    for k in range(2, alpha + 1):
        c = (k * k - k) / (2.0 * z * z)
        log_expm1 = c + math.log1p(-math.exp(-c)) if c > 1.0 else math.log(math.expm1(c))
        log_binom = lg(alpha + 1) - lg(k + 1) - lg(alpha - k + 1)
        log_excess = _log_add(log_excess, log_binom + (alpha - k) * log_1q + k * log_q + log_expm1)
    log_a = math.log1p(math.exp(log_excess)) if log_excess < 0.0 else log_excess + math.log1p(math.exp(-log_excess))
    return log_a / (alpha - 1)


def rdp_curve(z: float, q: float = 1.0, orders=ORDERS) -> list[float]:
    return [rdp_sampled_gaussian(a, z, q) for a in orders]


def epsilon_from_rdp(rdp, rounds: int, delta: float, orders=ORDERS) -> float:
    """min over the orders of rounds · rdp(α) + ln(1/δ) / (α − 1)."""
    if not 0.0 < delta < 1.0:
        raise ValueError(f"delta must lie in (0, 1), got {delta}")
    if rounds <= 0:
        return 0.0
    log_inv_delta = math.log(1.0 / delta)
    return min(rounds * r + log_inv_delta / (a - 1) for a, r in zip(orders, rdp))


def epsilon(z: float, rounds: int, delta: float, q: float = 1.0, orders=ORDERS) -> float:
    """ε of `rounds` compositions at noise multiplier z and failure probability δ. q = 1 (default): no
    amplification, valid for any participation scheme. q < 1: valid only for Poisson sampling at rate
    q (see the module docstring). z = 0 (no noise) gives inf."""
    if z <= 0:
        return math.inf if rounds > 0 and q > 0 else 0.0
    return epsilon_from_rdp(rdp_curve(z, q, orders), rounds, delta, orders)
