"""Shared by the GroupNorm tests (test_groupnorm_oracle.py, test_groupnorm_gpu.py): a float64
oracle written out plainly, and the input builders.

Activations are channels-last [K, B, H, W, C]; G groups of C / G adjacent channels; one statistic
per (client, sample, group). Everything here runs on the CPU in float64 (`ops.ref` computes in
fp32, so it is a path under test, not the oracle).
"""

import functools

import torch

from rowwise_common import F32_TOL, F32_TOL_DX, d

# (K, B, H, W, C, G, Kw): the smallest shapes at which each path of csrc/groupnorm.hip can go wrong
SHAPES = [
    (2, 3, 8, 8, 64, 2, None),    # base case
    (2, 3, 8, 8, 64, 32, None),   # Cg = 2: a 4-channel vector spans two groups
    (2, 3, 8, 8, 64, 64, None),   # Cg = 1
    (2, 3, 8, 8, 64, 1, None),    # a single group
    (2, 3, 4, 4, 512, 2, None),   # ResNet-18 layer4, Cg = 256: four pixel lanes per channel chunk
    (2, 2, 5, 5, 6, 3, None),     # C % 4 != 0 (scalar path), odd pixel count, idle threads
    (1, 2, 32, 32, 64, 2, None),  # 32,768 elements per group: every loop's second trip
    (3, 2, 16, 16, 128, 2, 1),    # shared γ / β (Kw = 1)
]
SHAPE_IDS = ["base", "cg2", "cg1", "g1", "l4", "c6", "l1", "shared"]

# The offset case: x of mean 64, std 1 at (1, 2, 32, 32, 64), G = 2. A one-pass variance
# (Σx²/n − mean²) errs by about 1e-4 there; fp32 itself cannot hold 1e-5, because x − mean is
# formed from values whose spacing is 7.6e-6. The bounds are max(tolerance, 4 × the error the
# fp32 CPU path `ops.ref` shows on this input), the ADAM_UPDATE_TOL precedent (the factor covers
# the summation-order freedom a correct fp32 kernel has).
#   measured, fp32 ops.ref.gn_fwd / gn_bwd (CPU) on offset_inputs(), rel_err against float64:
#     y 8.12e-06  mean 4.56e-07  rstd 3.29e-07  dx 3.77e-07  dgamma 2.40e-05  dbeta 1.20e-07
#   measured, gn_fwd_kernel / gn_bwd_kernel (MI355X), same input (the backward oracle is given the
#   kernel's own mean / rstd, so dγ carries no mean error there):
#     y 7.32e-07  mean 3.87e-08  rstd 4.11e-08  dx 1.19e-07  dgamma 1.59e-07  dbeta 1.54e-07
#   (dγ: the mean is off by 4.56e-7 · 64 = 2.9e-5, which shifts every x̂ by that much: Σĝ·x̂ moves by
#   2.9e-5 · |Σĝ| ≈ 1.3e-3 against max |dγ| ≈ 55. The backward is given the path's own fp32 mean.)
OFFSET_SHAPE = (1, 2, 32, 32, 64, 2)
OFFSET_REF_ERR = {"y": 8.12e-6, "mean": 4.56e-7, "rstd": 3.29e-7, "dx": 3.77e-7, "dgamma": 2.40e-5,
                  "dbeta": 1.20e-7}
OFFSET_TOL = {k: max(F32_TOL_DX if k == "dx" else F32_TOL, 4 * e) for k, e in OFFSET_REF_ERR.items()}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gn_inputs(K, B, H, W, C, Kw=None, offset=0.0, seed=0, dtype=torch.float32):
    """x [K, B, H, W, C] = randn + offset, γ = 1 ± 0.5·randn and β [Kw or K, C], dy and a residual."""
    g = _gen(seed)
    Kw = K if Kw is None else Kw
    x = (torch.randn(K, B, H, W, C, generator=g) + offset).to(dtype)
    gamma = (torch.randn(Kw, C, generator=g) * 0.5 + 1).to(dtype)
    beta = torch.randn(Kw, C, generator=g).to(dtype)
    dy = torch.randn(K, B, H, W, C, generator=g).to(dtype)
    res = torch.randn(K, B, H, W, C, generator=g).to(dtype)
    return x, gamma, beta, dy, res


@functools.lru_cache(maxsize=1)
def offset_inputs():
    K, B, H, W, C, _ = OFFSET_SHAPE
    return gn_inputs(K, B, H, W, C, offset=64.0, seed=5)


def _per_client(p, K):
    p = d(p)
    return p.repeat_interleave(K // p.shape[0], dim=0)[:, None, None, None, :]


def _real(x, valid):
    """[K, B, 1, 1, 1] bool: sample b of client k is read (b < valid[k])."""
    K, B = x.shape[:2]
    if valid is None:
        return torch.ones(K, B, 1, 1, 1, dtype=torch.bool)
    return (torch.arange(B)[None, :] < valid.cpu().long()[:, None]).view(K, B, 1, 1, 1)


def gn_fwd64(x, gamma, beta, G, relu=False, residual=None, valid=None, eps=1e-5):
    """(y, mean [K, B, G], rstd [K, B, G]) in float64; skipped samples: y = mean = rstd = 0."""
    x = d(x)
    K, B, H, W, C = x.shape
    m = _real(x, valid)
    x = torch.where(m, x, torch.zeros((), dtype=torch.float64))
    xg = x.reshape(K, B, H * W, G, C // G)
    mean = xg.mean(dim=(2, 4))
    var = ((xg - mean[:, :, None, :, None]) ** 2).mean(dim=(2, 4))
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((xg - mean[:, :, None, :, None]) * rstd[:, :, None, :, None]).reshape(x.shape)
    y = xhat * _per_client(gamma, K) + _per_client(beta, K)
    if residual is not None:
        y = y + torch.where(m, d(residual), torch.zeros((), dtype=torch.float64))
    if relu:
        y = y.clamp_min(0.0)
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(m, y, zero), torch.where(m.view(K, B, 1), mean, zero), torch.where(m.view(K, B, 1), rstd, zero)


def gn_bwd64(dy, x, gate, mean, rstd, gamma, G, valid=None):
    """(dx, dgamma [K, C], dbeta [K, C], dres) in float64. `gate`: bool tensor (True where the
    gradient passes: the ReLU gate y > 0 of the implementation under test) or None."""
    dy, x, mean, rstd = d(dy), d(x), d(mean), d(rstd)
    K, B, H, W, C = x.shape
    m = _real(x, valid)
    zero = torch.zeros((), dtype=torch.float64)
    g = torch.where(m, dy, zero)
    x = torch.where(m, x, zero)
    if gate is not None:
        g = torch.where(gate.cpu() & m, g, zero)
    xh = (x.reshape(K, B, H * W, G, C // G) - mean[:, :, None, :, None]) * rstd[:, :, None, :, None]
    xhat = torch.where(m, xh.reshape(x.shape), zero)
    dgamma = (g * xhat).sum(dim=(1, 2, 3))
    dbeta = g.sum(dim=(1, 2, 3))
    gg = (g * _per_client(gamma, K)).reshape(K, B, H * W, G, C // G)
    xh = xhat.reshape(K, B, H * W, G, C // G)
    dx = rstd[:, :, None, :, None] * (gg - gg.mean(dim=(2, 4), keepdim=True)
                                      - xh * (gg * xh).mean(dim=(2, 4), keepdim=True))
    return torch.where(m, dx.reshape(x.shape), zero), dgamma, dbeta, g


def poison_skipped(valid, *tensors):
    """Copies of the tensors with NaN in every sample b >= valid[k]: nothing may read them."""
    out = []
    for t in tensors:
        t = t.clone()
        for k, n in enumerate(valid.tolist()):
            t[k, n:] = float("nan")
        out.append(t)
    return out


def batch_composition_inputs():
    """K = 2, B = 4 CIFAR batches (a, b): b keeps sample 0 of each client and replaces samples 1–3."""
    g = _gen(21)
    a = torch.randn(2, 4, 32, 32, 3, generator=g)
    b = a.clone()
    b[:, 1:] = 3.0 * torch.randn(2, 3, 32, 32, 3, generator=g) + 1.0
    return a, b
