"""Shared by tests/test_rowwise_gpu.py and tests/test_rowwise_oracle.py: float64 oracles of the
row-wise kernels (LayerNorm, SGD / Adam steps, weighted sums, block norms, column sums), the
input builders of both files, and the error metric of tests/test_kernels_f32_gpu.py.

Everything here runs on the CPU in float64 and is written out plainly (`ops.ref` casts to fp32 in
places, so it is the fp32 CPU path under test in test_rowwise_oracle.py, not the oracle).
"""

import functools

import torch

F32_TOL = 1e-5  # fp32 kernels against float64 (README), LayerNorm dx at 2e-5
F32_TOL_DX = 2e-5
BF16_TOL = 2e-2  # bf16 kernels against ops.ref on the upcast inputs, LayerNorm dx at 3e-2
BF16_TOL_DX = 3e-2
SUM_TOL = 1e-12  # fp64 accumulators against the float64 oracle in the same k order
STEP_RTOL, STEP_ATOL = 1e-5, 1e-6  # optimiser steps (the bound of test_sgd_and_fl_math)

# Adam's update Δθ = θ_new − θ_old: max |Δθ − Δθ_exact| / max |Δθ_exact| per client row. The bound is
# four times what fp32 `ref.adam_step` gives on adam_inputs() (the factor covers the FMA and
# division-order freedom a correct fp32 kernel has). The error comes from β₂ = 0.999 itself, which
# fp32 holds 1.3e-8 high: 1 − β₂ᵗ is then off by 1.3e-5 at t = 1 and by 7.5e-6 at t = 1000.
#   measured, fp32 ref.adam_step (CPU), rows t = 1 / 2 / 1000:
#     weight decay 0: 8.21e-6 / 1.01e-5 / 9.53e-6    weight decay 1e-4: 7.25e-6 / 1.01e-5 / 9.51e-6
#   measured, adam_kernel (MI355X, __powf bias corrections), same rows:
#     weight decay 0: 7.07e-6 / 8.27e-6 / 9.53e-6    weight decay 1e-4: 7.25e-6 / 8.31e-6 / 9.51e-6
ADAM_REF_ERR = 1.01e-5  # the largest of the reference's figures above
ADAM_UPDATE_TOL = 4 * ADAM_REF_ERR


def d(t):
    return t.detach().cpu().double()


def rel_err(out, exact) -> float:
    """max |out − exact| / max |exact| on CPU doubles (the scale of the output)."""
    out, exact = d(out), d(exact)
    assert out.shape == exact.shape, (out.shape, exact.shape)
    return (out - exact).abs().max().item() / (exact.abs().max().item() + 1e-300)


def close(out, exact, tol, what=""):
    e = rel_err(out, exact)
    assert e <= tol, f"{what} rel err {e:.3g} > {tol}"
    return e


def bits_equal(a, b) -> bool:
    """Same shape, dtype and bit pattern (NaN payloads and the sign of zero included)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------ LayerNorm
def ln_inputs(K, rows, C, Kw=None, mean=0.0, seed=0, dtype=torch.float32):
    """x [K, rows, C] with rows of the given mean and std 1, γ ≈ 1 and β [Kw or K, C], dy."""
    g = _gen(seed)
    Kw = K if Kw is None else Kw
    x = (torch.randn(K, rows, C, generator=g) + mean).to(dtype)
    gamma = (torch.randn(Kw, C, generator=g) * 0.5 + 1).to(dtype)
    beta = torch.randn(Kw, C, generator=g).to(dtype)
    dy = torch.randn(K, rows, C, generator=g).to(dtype)
    return x, gamma, beta, dy


def _per_client(p, K):
    p = d(p)
    return p.repeat_interleave(K // p.shape[0], dim=0)[:, None, :]


def ln_fwd64(x, gamma, beta, eps=1e-5):
    x = d(x)
    K = x.shape[0]
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[..., None]) * rstd[..., None] * _per_client(gamma, K) + _per_client(beta, K)
    return y, mean, rstd


def ln_bwd64(dy, x, mean, rstd, gamma):
    dy, x, mean, rstd = d(dy), d(x), d(mean), d(rstd)
    K = x.shape[0]
    xhat = (x - mean[..., None]) * rstd[..., None]
    dgamma = (dy * xhat).sum(1)
    dbeta = dy.sum(1)
    gg = dy * _per_client(gamma, K)
    dx = rstd[..., None] * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))
    return dx, dgamma, dbeta


# ------------------------------------------------------------------ optimiser steps
SGD_SETTINGS = [  # momentum, dampening, nesterov, weight decay
    (0.0, 0.0, False, 0.0),
    (0.0, 0.0, False, 5e-4),
    (0.9, 0.0, True, 5e-4),
    (0.9, 0.1, False, 0.0),
    (0.5, 0.0, True, 0.0),
]
SGD_P = 3 * 1048576 + 80  # 1024 workgroups x 256 threads x 2 float4: a second, ragged trip
SGD_ACTIVE = [1, 0, 1]
SGD_FIRST = [0, 0, 1]


@functools.lru_cache(maxsize=2)
def sgd_inputs(P=SGD_P):
    """θ, grad, momentum [3, P] fp32 and lr [3]: row 1 inactive, row 2 on its first step."""
    g = _gen(11)
    theta = torch.randn(3, P, generator=g)
    grad = torch.randn(3, P, generator=g)
    mom = torch.randn(3, P, generator=g)
    lr = torch.tensor([0.05, 0.3, 0.011])
    return theta, grad, mom, lr


def sgd_step64(theta, grad, mom, lr, active, first, momentum, dampening, nesterov, wd):
    """torch.optim.SGD's step on float64 copies; returns (θ_new, momentum_new)."""
    t, g, m, lr = d(theta), d(grad), d(mom), d(lr)[:, None]
    a = torch.tensor(active, dtype=torch.bool)[:, None]
    fs = torch.tensor(first, dtype=torch.bool)[:, None]
    g = g + wd * t
    if momentum != 0:
        buf = torch.where(fs, g, momentum * m + (1 - dampening) * g)
        m = torch.where(a, buf, m)
        g = g + momentum * buf if nesterov else buf
    return torch.where(a, t - lr * g, t), m


@functools.lru_cache(maxsize=8)
def sgd_expected(setting, P=SGD_P):
    theta, grad, mom, lr = sgd_inputs(P)
    return sgd_step64(theta, grad, mom, lr, SGD_ACTIVE, SGD_FIRST, *setting)


ADAM_P = 2 * 262144 + 48  # 1024 workgroups x 256 threads: two full trips and a ragged third
ADAM_ACTIVE = [1, 1, 0, 1]
ADAM_STEP = [1, 2, 10, 1000]
ADAM_HYPER = (0.9, 0.999, 1e-8)  # β₁, β₂, ε


@functools.lru_cache(maxsize=1)
def adam_inputs(P=ADAM_P):
    g = _gen(12)
    theta = torch.randn(4, P, generator=g)
    grad = torch.randn(4, P, generator=g)
    m = torch.randn(4, P, generator=g) * 0.1
    v = torch.rand(4, P, generator=g) * 0.01 + 1e-6
    lr = torch.tensor([1e-3, 3e-3, 1e-2, 5e-4])
    return theta, grad, m, v, lr


def adam_step64(theta, grad, m, v, lr, active, step, wd, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's step (L2 weight decay) on float64 copies; returns (θ_new, m_new, v_new)."""
    t, g, m, v, lr = d(theta), d(grad), d(m), d(v), d(lr)[:, None]
    a = torch.tensor(active, dtype=torch.bool)[:, None]
    n = torch.tensor(step, dtype=torch.float64)[:, None]
    g = g + wd * t
    mn = beta1 * m + (1 - beta1) * g
    vn = beta2 * v + (1 - beta2) * g * g
    new = t - lr * (mn / (1 - beta1 ** n)) / (torch.sqrt(vn / (1 - beta2 ** n)) + eps)
    return torch.where(a, new, t), torch.where(a, mn, m), torch.where(a, vn, v)


@functools.lru_cache(maxsize=2)
def adam_expected(wd):
    theta, grad, m, v, lr = adam_inputs()
    return adam_step64(theta, grad, m, v, lr, ADAM_ACTIVE, ADAM_STEP, wd, *ADAM_HYPER)


def update_err(theta_new, theta_old, theta_exact):
    """Per client row: max |Δθ − Δθ_exact| / max |Δθ_exact| with Δθ = θ_new − θ_old in float64."""
    du, de = d(theta_new) - d(theta_old), d(theta_exact) - d(theta_old)
    return (du - de).abs().amax(1) / de.abs().amax(1).clamp_min(1e-300)


def guarded(rows, pad=16, sentinel=7.0):
    """(wide, view): `rows` [K, P] copied into the first P columns of a [K, P + pad] buffer whose
    guard columns hold `sentinel`; the view has row stride P + pad."""
    K, P = rows.shape
    wide = torch.full((K, P + pad), sentinel, dtype=rows.dtype, device=rows.device)
    wide[:, :P] = rows
    return wide, wide[:, :P]


# ------------------------------------------------------------------------ reductions
def weighted_sum64(x, w, out):
    """out + w_0 x_0 + w_1 x_1 + … in float64, added in that order (the kernel's)."""
    acc = d(out).clone()
    for k in range(x.shape[0]):
        acc += float(w[k]) * d(x[k])
    return acc


def masked_weighted_sum64(x, mask, w, num, den):
    n, dn = d(num).clone(), d(den).clone()
    for k in range(x.shape[0]):
        mk = mask[k].cpu().bool()
        n += torch.where(mk, float(w[k]) * d(x[k]), torch.zeros(()).double())
        dn += torch.where(mk, torch.full((), float(w[k])).double(), torch.zeros(()).double())
    return n, dn


# One repeat of the block pattern (elements; −n = a gap of n elements with id −1). A wave covers
# 64 chunks of 16 = 1024 elements, a workgroup 4096. In the first repeat: 1024 fills one wave
# exactly; 16 and 32 sit inside a wave; 1008 and 1040 start and end inside waves and cross one wave
# boundary each; 4800 crosses a workgroup boundary; 65,536 starts and ends on workgroup boundaries
# and spans 16 workgroups. A repeat is 4609 chunks, so every later repeat is shifted by one more
# chunk against the waves.
BLOCK_PATTERN = [1024, 16, 32, -16, 1008, 1040, 4800, -256, 65536, 16]
BLOCK_REPEATS = 57  # 57 x 73,744 = 4,203,408 > 4,194,304 = 1024 workgroups x 256 chunks x 16


@functools.lru_cache(maxsize=1)
def block_layout():
    """(ids [P] int32, offsets [nb + 1] int64, sizes [nb] int64) of BLOCK_REPEATS patterns."""
    ids, sizes, b = [], [], 0
    for _ in range(BLOCK_REPEATS):
        for n in BLOCK_PATTERN:
            if n < 0:
                ids.append(torch.full((-n,), -1, dtype=torch.int32))
            else:
                ids.append(torch.full((n,), b, dtype=torch.int32))
                sizes.append(n)
                b += 1
    sizes = torch.tensor(sizes)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    return torch.cat(ids), offsets, sizes


@functools.lru_cache(maxsize=1)
def block_inputs():
    ids, _, _ = block_layout()
    return torch.randn(2, ids.numel(), generator=_gen(13))


@functools.lru_cache(maxsize=1)
def block_sq64():
    """Σx² of every (row, block) in float64; gaps (id −1) belong to no block."""
    ids, _, sizes = block_layout()
    x = block_inputs()
    valid = ids >= 0
    out = torch.zeros(x.shape[0], sizes.numel(), dtype=torch.float64)
    out.index_add_(1, ids[valid].long(), d(x[:, valid]) ** 2)
    return out


def block_starts():
    """First element of every block, in block order."""
    ids, _, _ = block_layout()
    first = torch.ones_like(ids, dtype=torch.bool)
    first[1:] = ids[1:] != ids[:-1]
    return torch.nonzero(first & (ids >= 0)).flatten().tolist()


def seq_sum_tol(sizes):
    """Relative error allowed to an fp32 sum of n positive terms added one after another (the CPU
    path's index_add_): every add rounds the running sum by at most u = 2^-24 of itself, a random
    walk of n steps; 4·u·√n is four standard deviations of it with the squares' own rounding
    included (6.1e-5 at n = 65,536, 9.5e-7 at n = 16)."""
    return 4 * 2.0 ** -24 * torch.as_tensor(sizes, dtype=torch.float64).sqrt()


def block_err(out, exact) -> float:
    """Largest relative error of any single block (all terms are positive)."""
    return ((d(out) - exact).abs() / exact).max().item()


SEG_BOUNDS = [0, 1, 63, 64, 65, 255, 257, 1000, 1024, 1300, 2047, 2049, 3000, 3500, 3900, 4096, 4112]
SEG_CLASSES = ["neg", "pos", "mixed", "pzero", "nzero", "denorm", "neg_nzero", "pos_nzero"]


def seg_inputs():
    """x [2, 4112], seg ids [4112], nseg: every value class in segments of several lengths. Row 1
    has the classes shifted by three segments, so each lands on other boundaries. The single-element
    segments ([0, 1), [63, 64), [64, 65)) are the 'single element' class whatever they hold."""
    g = _gen(14)
    P, nseg = SEG_BOUNDS[-1], len(SEG_BOUNDS) - 1
    seg = torch.empty(P, dtype=torch.int32)
    x = torch.empty(2, P)
    for s in range(nseg):
        lo, hi = SEG_BOUNDS[s], SEG_BOUNDS[s + 1]
        seg[lo:hi] = s
        for k in range(2):
            n = hi - lo
            r = torch.randn(n, generator=g)
            cls = SEG_CLASSES[(s + 3 * k) % len(SEG_CLASSES)]
            if cls == "neg":
                v = -r.abs() - 0.01
            elif cls == "pos":
                v = r.abs() + 0.01
            elif cls == "mixed":
                v = r
            elif cls == "pzero":
                v = torch.zeros(n)
            elif cls == "nzero":
                v = -torch.zeros(n)
            elif cls == "denorm":
                v = r * 1e-41
            else:  # −0.0 in the first half (the first waves of a long segment), one sign in the rest
                v = -r.abs() - 0.01 if cls == "neg_nzero" else r.abs() + 0.01
                v[: max(1, n // 2)] = -0.0
            x[k, lo:hi] = v
    return x, seg, nseg


def seg_minmax_exact(x, seg, nseg):
    x = x.cpu()
    mn = torch.stack([torch.stack([x[k, seg == s].amin() for s in range(nseg)]) for k in range(x.shape[0])])
    mx = torch.stack([torch.stack([x[k, seg == s].amax() for s in range(nseg)]) for k in range(x.shape[0])])
    return mn, mx


def col_inputs(rows, C, dtype, seed=15):
    return torch.randn(2, rows, C, generator=_gen(seed)).to(dtype)


def col_sum64(dy):
    return d(dy).sum(1)
