"""Plain-PyTorch reference implementations of every client-batched primitive.

These are the numerics oracles for the HIP kernels (tests compare `ops.hip.*` against
`ops.ref.*` computed in fp32) and the CPU execution path used by the CPU test-suite.
Shapes follow the cohort layout used everywhere in this framework:

  images  x  [K, B, H, W, C]      (K = clients resident on the rank, NHWC per client)
  conv w     [K, Co, kh, kw, Ci]
  linear x   [K, N, Fi], w [K, Fo, Fi], b [K, Fo]
  bn x       [K, R, C]  (R = B*H*W rows, per-client batch statistics)

The reference never fuses anything (eager PyTorch inside cyy_torch_toolbox); the inventory
of implicit compute sites these replace is SURVEY §2.5 (K1-K23).
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _match(w, K: int):
    """Weights are [M, ...] for K = M*rep virtual clients (rep clients share one weight
    row: evaluation of one model over many test batches, GTG subset models, ...)."""
    if w is None or w.shape[0] == K:
        return w
    assert K % w.shape[0] == 0, (K, w.shape)
    return w.repeat_interleave(K // w.shape[0], dim=0)


# ----------------------------------------------------------------------------- conv
# A client's bits must not depend on who shares its cohort (N ranks ≡ 1 rank), so torch has to pick
# the same convolution kernels for every K. Two things stood in the way. Left to `reshape`, a lone
# client's input (K = 1) and a contiguous weight come out as channels-last VIEWS, a cohort's input
# and a weight that is a strided view of θ as NCHW copies: both operands are now always contiguous
# NCHW copies. And groups = 1 takes other kernels than groups > 1: a lone client is run as two
# identical groups (`_twice`) and the first is kept.
def _to_grouped(x: torch.Tensor) -> torch.Tensor:
    K, B, H, W, C = x.shape
    return x.permute(1, 0, 4, 2, 3).reshape(B, K * C, H, W).contiguous()


def _from_grouped(y: torch.Tensor, K: int) -> torch.Tensor:
    B, KC, H, W = y.shape
    return y.reshape(B, K, KC // K, H, W).permute(1, 0, 3, 4, 2)


def _w_grouped(w: torch.Tensor) -> torch.Tensor:
    K, Co, kh, kw, Ci = w.shape
    return w.permute(0, 1, 4, 2, 3).reshape(K * Co, Ci, kh, kw).contiguous()


def _twice(t):
    return torch.cat([t, t])


def conv_fwd(x, w, stride: int, pad: int, bias=None):
    K = x.shape[0]
    if K == 1:
        return conv_fwd(_twice(x), w, stride, pad, bias)[:1]
    w = _match(w, K)
    b = _match(bias, K).reshape(-1).to(x.dtype) if bias is not None else None
    y = F.conv2d(_to_grouped(x), _w_grouped(w).to(x.dtype), b, stride=stride, padding=pad, groups=K)
    return _from_grouped(y, K).contiguous()


def conv_dgrad(dy, w, in_hw, stride: int, pad: int, acc=None):
    K, B = dy.shape[:2]
    if K == 1:
        dx = conv_dgrad(_twice(dy), w, in_hw, stride, pad)[:1]
        return dx if acc is None else dx + acc.to(dx.dtype)
    w = _match(w, K)
    Ci = w.shape[-1]
    dx = torch.nn.grad.conv2d_input(
        (B, K * Ci, in_hw[0], in_hw[1]), _w_grouped(w), _to_grouped(dy),
        stride=stride, padding=pad, groups=K,
    )
    dx = _from_grouped(dx, K).contiguous()
    return dx if acc is None else dx + acc.to(dx.dtype)


def conv_wgrad(dy, x, w_shape, stride: int, pad: int):
    K = x.shape[0]
    if K == 1:
        return conv_wgrad(_twice(dy), _twice(x), w_shape, stride, pad)[:1]
    _, Co, kh, kw, Ci = w_shape
    dw = torch.nn.grad.conv2d_weight(
        _to_grouped(x), (K * Co, Ci, kh, kw), _to_grouped(dy),
        stride=stride, padding=pad, groups=K,
    )
    return dw.reshape(K, Co, Ci, kh, kw).permute(0, 1, 3, 4, 2)


# ---------------------------------------------------------------------------- linear
def dropout_keep(K: int, rows: int, N: int, seeds, p: float) -> torch.Tensor:
    """[K, rows, N] keep mask of the GEMM-epilogue dropout (common.h drop_keep):
    mix32(m·N + n, seed_k) >= p·2^32."""
    import numpy as np

    from .fl import _mix

    thr = int(min(float(np.float32(p) * np.float32(4294967296.0)), 4294967040.0))
    idx = torch.arange(rows * N, dtype=torch.int64, device=seeds.device).view(1, rows * N)
    sk = (seeds.long() & 0xFFFFFFFF).view(K, 1)
    return (_mix(idx, sk) >= thr).view(K, rows, N)


def dropout_apply(x, seeds, p: float):
    K, N = x.shape[0], x.shape[-1]
    keep = dropout_keep(K, x.numel() // (K * N), N, seeds.to(x.device), p).view(x.shape)
    return torch.where(keep, x * (1.0 / (1.0 - p)), torch.zeros_like(x))


def linear_fwd(x, w, b=None, relu=False, acc=None, drop_p: float = 0.0, drop_seeds=None):
    K = x.shape[0]
    w = _match(w, K)
    y = torch.bmm(x, w.transpose(1, 2))
    if b is not None:
        b = _match(b, K)
        y = y + b[:, None, :]
    if relu:
        y = torch.relu(y)
    if drop_p:
        y = dropout_apply(y, drop_seeds, drop_p)
    if acc is not None:
        y = y.to(acc.dtype) + acc
    return y


def linear_dgrad(dy, w, gate=None, gate_scale: float = 1.0):
    K = dy.shape[0]
    w = _match(w, K)
    dx = torch.bmm(dy, w)
    if gate_scale != 1.0:
        dx = dx * gate_scale
    return dx if gate is None else dx * (gate > 0).to(dx.dtype)


def linear_wgrad(dy, x, with_bias: bool):
    dw = torch.bmm(dy.transpose(1, 2), x)
    db = dy.sum(dim=1) if with_bias else None
    return dw, db


# ------------------------------------------------------------------------ batch norm
def _row_mask(R: int, valid_rows, device):
    if valid_rows is None:
        return None
    ar = torch.arange(R, device=device)
    return (ar[None, :] < valid_rows[:, None].to(device)).unsqueeze(-1)  # [K,R,1]


def bn_fwd(x, gamma, beta, valid_rows=None, relu=False, residual=None, eps=1e-5):
    """Training-mode BN with batch statistics over valid rows (reference disables running
    stats: `util/model.py:23`, `server.py:48`), + optional residual add and ReLU."""
    K, R, C = x.shape
    xf = x.float()
    m = _row_mask(R, valid_rows, x.device)
    if m is None:
        n = torch.full((K, 1), float(R), device=x.device)
        mean = xf.mean(dim=1)
        var = ((xf - mean[:, None]) ** 2).mean(dim=1)
    else:
        n = valid_rows.to(x.device).float().clamp(min=1).unsqueeze(1)
        mean = (xf * m).sum(dim=1) / n
        var = (((xf - mean[:, None]) ** 2) * m).sum(dim=1) / n
    rstd = torch.rsqrt(var + eps)
    gamma, beta = _match(gamma, K), _match(beta, K)
    y = (xf - mean[:, None]) * rstd[:, None] * gamma.float()[:, None] + beta.float()[:, None]
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = torch.relu(y)
    if m is not None:
        y = y * m
    return y.to(x.dtype), mean, rstd


def bn_bwd(dy, x, y, mean, rstd, gamma, valid_rows=None, relu=False):
    """Returns (dx, dgamma, dbeta, dpre) where dpre = dL/d(bn_out + residual)."""
    K, R, C = x.shape
    m = _row_mask(R, valid_rows, x.device)
    g = dy.float()
    if relu:
        g = g * (y.float() > 0)
    if m is not None:
        g = g * m
        n = valid_rows.to(x.device).float().clamp(min=1).unsqueeze(1)
    else:
        n = torch.full((K, 1), float(R), device=x.device)
    xhat = (x.float() - mean[:, None]) * rstd[:, None]
    if m is not None:
        xhat = xhat * m
    dbeta = g.sum(dim=1)
    dgamma = (g * xhat).sum(dim=1)
    gamma = _match(gamma, K)
    dx = gamma.float()[:, None] * rstd[:, None] * (
        g - dbeta[:, None] / n[:, None] - xhat * dgamma[:, None] / n[:, None]
    )
    if m is not None:
        dx = dx * m
    return dx.to(x.dtype), dgamma, dbeta, g.to(x.dtype)


# ------------------------------------------------------------------------ layer norm
def ln_fwd(x, gamma, beta, eps=1e-5):
    K = x.shape[0]
    xf = x.float()
    mean = xf.mean(dim=-1)
    var = ((xf - mean[..., None]) ** 2).mean(dim=-1)
    rstd = torch.rsqrt(var + eps)
    gamma, beta = _match(gamma, K), _match(beta, K)
    shape = (K,) + (1,) * (x.dim() - 2) + (x.shape[-1],)
    y = (xf - mean[..., None]) * rstd[..., None] * gamma.float().reshape(shape) + beta.float().reshape(shape)
    return y.to(x.dtype), mean, rstd


def ln_bwd(dy, x, mean, rstd, gamma):
    K = x.shape[0]
    C = x.shape[-1]
    gamma = _match(gamma, K)
    shape = (K,) + (1,) * (x.dim() - 2) + (C,)
    g = dy.float()
    xhat = (x.float() - mean[..., None]) * rstd[..., None]
    red = tuple(range(1, x.dim() - 1))
    dgamma = (g * xhat).sum(dim=red)
    dbeta = g.sum(dim=red)
    gg = g * gamma.float().reshape(shape)
    dx = rstd[..., None] * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))
    return dx.to(x.dtype), dgamma, dbeta


# ------------------------------------------------------------------------ group norm
def _sample_mask(x, valid):
    """[K, B, 1, ..., 1] bool: sample b of client k is real (b < valid[k]); None without `valid`."""
    if valid is None:
        return None
    K, B = x.shape[:2]
    m = torch.arange(B, device=x.device)[None, :] < valid.to(x.device)[:, None]
    return m.view((K, B) + (1,) * (x.dim() - 2))


def _gn_params(p, K: int, dim: int):
    p = _match(p, K).float()
    return p.reshape((K,) + (1,) * (dim - 2) + (p.shape[-1],))


def gn_fwd(x, gamma, beta, G: int, valid=None, relu=False, residual=None, eps=1e-5):
    """GroupNorm of channels-last x [K, B, ..., C]: G groups of C / G adjacent channels, one
    (mean, biased two-pass variance) per (client, sample, group); then + residual, then ReLU.
    `valid` [K]: samples b >= valid[k] are not read (they may hold anything, NaN included); their
    y is +0 and their mean / rstd are 0. Returns (y, mean [K, B, G], rstd [K, B, G])."""
    K, B, C = x.shape[0], x.shape[1], x.shape[-1]
    assert C % G == 0, (C, G)
    m = _sample_mask(x, valid)
    xf = x.float()
    if m is not None:
        xf = torch.where(m, xf, torch.zeros((), device=x.device))
    xg = xf.reshape(K, B, -1, G, C // G)
    mean = xg.mean(dim=(2, 4))
    var = ((xg - mean[:, :, None, :, None]) ** 2).mean(dim=(2, 4))
    rstd = torch.rsqrt(var + eps)
    xhat = ((xg - mean[:, :, None, :, None]) * rstd[:, :, None, :, None]).reshape(x.shape)
    y = xhat * _gn_params(gamma, K, x.dim()) + _gn_params(beta, K, x.dim())
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = torch.relu(y)
    if m is not None:
        zero = torch.zeros((), device=x.device)
        y = torch.where(m, y, zero)
        mean = torch.where(m.view(K, B, 1), mean, zero)
        rstd = torch.where(m.view(K, B, 1), rstd, zero)
    return y.to(x.dtype), mean, rstd


def gn_bwd(dy, x, y, mean, rstd, gamma, G: int, valid=None, relu=False, need_dres=False):
    """Returns (dx, dgamma [K, C], dbeta [K, C], dres): ĝ = dy·[y > 0] with ReLU (`y` may be the
    output or any tensor positive exactly where it is), dres = ĝ (None unless `need_dres`). Samples
    b >= valid[k] are not read: dx = dres = +0 there and they add nothing to dγ / dβ."""
    K, B, C = x.shape[0], x.shape[1], x.shape[-1]
    m = _sample_mask(x, valid)
    g = dy.float()
    xf = x.float()
    if relu:
        g = g * (y.float() > 0)
    if m is not None:
        zero = torch.zeros((), device=x.device)
        g = torch.where(m, g, zero)
        xf = torch.where(m, xf, zero)
    xhat = ((xf.reshape(K, B, -1, G, C // G) - mean[:, :, None, :, None]) * rstd[:, :, None, :, None]).reshape(x.shape)
    red = tuple(range(1, x.dim() - 1))
    dgamma = (g * xhat).sum(dim=red)
    dbeta = g.sum(dim=red)
    gg = (g * _gn_params(gamma, K, x.dim())).reshape(K, B, -1, G, C // G)
    xh = xhat.reshape(K, B, -1, G, C // G)
    dx = rstd[:, :, None, :, None] * (gg - gg.mean(dim=(2, 4), keepdim=True)
                                      - xh * (gg * xh).mean(dim=(2, 4), keepdim=True))
    dx = dx.reshape(x.shape)
    if m is not None:
        dx = torch.where(m, dx, zero)
    return dx.to(x.dtype), dgamma, dbeta, (g.to(x.dtype) if need_dres else None)


# -------------------------------------------------------------------------- pooling
def maxpool_fwd(x, k: int, s: int, pad: int = 0):
    K, B, H, W, C = x.shape
    g = _to_grouped(x)
    y, idx = F.max_pool2d(g, k, s, padding=pad, return_indices=True)
    return _from_grouped(y, K).contiguous(), idx


def maxpool_bwd(dy, idx, x_shape, k: int, s: int, pad: int = 0):
    # scatter-ADD (overlapping windows, e.g. 3x3/s2, route several grads to one input;
    # max_unpool2d would overwrite instead of accumulate)
    K, B, H, W, C = x_shape
    g = _to_grouped(dy).float()
    out = torch.zeros((B, K * C, H * W), dtype=torch.float32, device=dy.device)
    out.scatter_add_(2, idx.flatten(2), g.flatten(2))
    return _from_grouped(out.view(B, K * C, H, W), K).to(dy.dtype).contiguous()


def avgpool_fwd(x, k: int, s: int):
    K = x.shape[0]
    return _from_grouped(F.avg_pool2d(_to_grouped(x), k, s), K).contiguous()


def avgpool_bwd(dy, x_shape, k: int, s: int):
    K, B, H, W, C = x_shape
    xg = torch.zeros((B, K * C, H, W), dtype=dy.dtype, device=dy.device, requires_grad=True)
    with torch.enable_grad():
        y = F.avg_pool2d(xg, k, s)
        (g,) = torch.autograd.grad(y, xg, _to_grouped(dy))
    return _from_grouped(g, K).contiguous()


def gap_fwd(x):
    """Global average pool [K,B,H,W,C] -> [K,B,C]."""
    return x.float().mean(dim=(2, 3)).to(x.dtype)


def gap_bwd(dy, x_shape):
    K, B, H, W, C = x_shape
    return (dy.float()[:, :, None, None, :] / (H * W)).expand(K, B, H, W, C).to(dy.dtype).contiguous()


# -------------------------------------------------------------------- cross entropy
def ce_fwd_bwd(logits, labels, valid=None):
    """Per-client mean softmax cross-entropy over valid samples, correct counts and the
    gradient dlogits (already divided by n_k). logits [K,B,C], labels [K,B] int."""
    K, B, C = logits.shape
    lf = logits.float()
    logp = torch.log_softmax(lf, dim=-1)
    nll = -logp.gather(-1, labels.long().unsqueeze(-1)).squeeze(-1)  # [K,B]
    if valid is None:
        m = torch.ones((K, B), device=logits.device)
        n = torch.full((K,), float(B), device=logits.device)
    else:
        m = (torch.arange(B, device=logits.device)[None, :] < valid[:, None].to(logits.device)).float()
        n = valid.to(logits.device).float().clamp(min=1)
    loss = (nll * m).sum(dim=1) / n
    correct = ((lf.argmax(-1) == labels.long()).float() * m).sum(dim=1)
    p = logp.exp()
    p.scatter_add_(-1, labels.long().unsqueeze(-1), -torch.ones_like(p[..., :1]))
    dlogits = p * (m / n[:, None]).unsqueeze(-1)
    return loss, correct, dlogits.to(logits.dtype)


# ----------------------------------------------------------------------- embedding
def embedding_fwd(tokens, table, scale: float = 1.0, pe=None):
    K = tokens.shape[0]
    table = _match(table, K)
    flat = tokens.reshape(K, -1).long()
    out = torch.gather(table, 1, flat.unsqueeze(-1).expand(-1, -1, table.shape[-1]))
    out = out.reshape(*tokens.shape, table.shape[-1])
    if scale != 1.0 or pe is not None:
        out = out.float() * scale
        if pe is not None:
            out = out + pe.to(out.device, torch.float32)
        out = out.to(table.dtype)
    return out


def embedding_bwd(dy, tokens, vocab: int, scale: float = 1.0):
    K = tokens.shape[0]
    D = dy.shape[-1]
    flat = tokens.reshape(K, -1).long()
    out = torch.zeros((K, vocab, D), dtype=torch.float32, device=dy.device)
    out.scatter_add_(1, flat.unsqueeze(-1).expand(-1, -1, D), dy.reshape(K, -1, D).float() * scale)
    return out


def seq_mean_fwd(x, lengths):
    L = x.shape[-2]
    m = (torch.arange(L, device=x.device) < lengths.to(x.device)[..., None]).to(torch.float32)
    return ((x.float() * m[..., None]).sum(-2) / lengths.to(x.device).clamp(min=1)[..., None].float()).to(x.dtype)


def seq_mean_bwd(dy, lengths, L: int):
    m = (torch.arange(L, device=dy.device) < lengths.to(dy.device)[..., None]).to(torch.float32)
    g = dy.float()[..., None, :] * m[..., None] / lengths.to(dy.device).clamp(min=1)[..., None, None].float()
    return g.to(dy.dtype)


# ----------------------------------------------------------------------- attention
def attn_drop_scale(shape, seeds, p: float, device) -> torch.Tensor:
    """[K,B,Hh,L,L] attention-probability dropout factor M/(1−p) (attention_mfma.hip attn_keep):
    keep iff mix32(((b·Hh + h)·L + q)·L + key, seed_k) >= p·2³² (32-bit index)."""
    import numpy as np

    from .fl import _mix

    K, B, Hh, L = shape[:4]
    thr = int(min(float(np.float32(p) * np.float32(4294967296.0)), 4294967040.0))
    hl = torch.arange(B * Hh, dtype=torch.int64, device=device).view(B, Hh, 1, 1)
    qi = torch.arange(L, dtype=torch.int64, device=device).view(1, 1, L, 1)
    kj = torch.arange(L, dtype=torch.int64, device=device).view(1, 1, 1, L)
    idx = ((hl * L + qi) * L + kj) & 0xFFFFFFFF
    sk = (seeds.long().to(device) & 0xFFFFFFFF).view(K, 1, 1, 1, 1)
    keep = _mix(idx.unsqueeze(0), sk) >= thr
    return keep.float() * (1.0 / (1.0 - p))


def attn_fwd(q, k, v, key_valid=None, drop_p: float = 0.0, drop_seeds=None):
    """q,k,v [K,B,Hh,L,dh]; key_valid [K,B] number of valid keys (padding mask) or None;
    drop_p / drop_seeds [K]: dropout on the attention probabilities (nn.MultiheadAttention's
    `dropout`). Returns o and the log-sum-exp [K,B,Hh,L] (fp32, of the undropped scores).
    A sequence without a valid key (key_valid = 0: an empty text) gives o = 0 and lse = 0, as the
    kernels do (csrc/attention*.hip `l > 0 ? … : 0`); with that lse `attn_bwd` gives it p = 0 and
    zero gradients."""
    scale = q.shape[-1] ** -0.5
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    empty = None
    if key_valid is not None:
        L = k.shape[-2]
        km = torch.arange(L, device=q.device)[None, None, :] < key_valid[..., None].to(q.device)
        s = s.masked_fill(~km[:, :, None, None, :], float("-inf"))
        empty = (key_valid.to(q.device) <= 0)[:, :, None, None]
    lse = torch.logsumexp(s, dim=-1)
    if empty is not None:
        lse = lse.masked_fill(empty, 0.0)  # (−inf there: exp(s − lse) would be NaN, now exp(−inf) = 0)
    p = torch.exp(s - lse[..., None])
    if drop_p:
        p = p * attn_drop_scale(q.shape, drop_seeds, drop_p, q.device)
    o = torch.matmul(p, v.float())
    return o.to(q.dtype), lse


def attn_bwd(do, q, k, v, o, lse, key_valid=None, drop_p: float = 0.0, drop_seeds=None):
    scale = q.shape[-1] ** -0.5
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if key_valid is not None:
        L = k.shape[-2]
        km = torch.arange(L, device=q.device)[None, None, :] < key_valid[..., None].to(q.device)
        s = s.masked_fill(~km[:, :, None, None, :], float("-inf"))
    p = torch.exp(s - lse[..., None])
    msk = attn_drop_scale(q.shape, drop_seeds, drop_p, q.device) if drop_p else None
    dof = do.float()
    dv = torch.matmul((p * msk if msk is not None else p).transpose(-1, -2), dof)
    dp = torch.matmul(dof, v.float().transpose(-1, -2))
    if msk is not None:
        dp = dp * msk
    delta = (dof * o.float()).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, k.float())
    dk = torch.matmul(ds.transpose(-1, -2), q.float())
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


# ------------------------------------------------------------------------- sparse
def spmm(rowptr, col, val, x):
    """CSR (shared graph) times per-client dense x [K,N,F] -> [K,N,F]."""
    N = rowptr.numel() - 1
    A = torch.sparse_csr_tensor(rowptr.long(), col.long(), val.float(), size=(N, x.shape[1]))
    return torch.stack([(A @ x[k].float()) for k in range(x.shape[0])]).to(x.dtype)


# ---------------------------------------------------------------- optimiser / FL math
def sgd_step(theta, grad, mom, lr, active, weight_decay, momentum, dampening, nesterov,
             first_step, shadow=None, split=None):
    """Fused SGD over flat [K,P] buffers (torch.optim.SGD semantics, per-client lr[K]).
    `first_step[k]` (bool) makes buf = g (torch initialises the momentum buffer with the
    first gradient). Inactive clients are left untouched."""
    a = active.to(theta.device).bool()
    g = grad + weight_decay * theta if weight_decay != 0 else grad.clone()
    if momentum != 0:
        fs = first_step.to(theta.device).bool()[:, None]
        buf = torch.where(fs, g, momentum * mom + (1 - dampening) * g)
        mom.copy_(torch.where(a[:, None], buf, mom))
        d = g + momentum * buf if nesterov else buf
    else:
        d = g
    new = theta - lr.to(theta.device).float()[:, None] * d
    theta.copy_(torch.where(a[:, None], new, theta))
    if shadow is not None:
        shadow.copy_(theta.to(shadow.dtype))
    if split is not None:
        split_rows(theta, split)


def sgd_step_corrected(theta, grad, mom, lr, active, weight_decay, momentum, dampening, nesterov, first_step, mu,
                       anchor, corr, shadow=None, split=None):
    """The drift-corrected step, literally: g' from separate fp32 elementwise operations (each
    rounded once), then `sgd_step` on it. `grad`, `corr` and `anchor` are not written."""
    g = grad
    if corr is not None:
        g = g + corr
    if mu != 0:
        assert anchor is not None, "mu != 0 needs the anchor row"
        d = theta - anchor.unsqueeze(0)
        d = d * float(mu)
        g = g + d
    sgd_step(theta, g, mom, lr, active, weight_decay, momentum, dampening, nesterov, first_step, shadow, split)


def adam_step(theta, grad, m, v, lr, active, step, beta1, beta2, eps, weight_decay, shadow=None):
    a = active.to(theta.device).bool()[:, None]
    g = grad + weight_decay * theta if weight_decay != 0 else grad
    m_new = beta1 * m + (1 - beta1) * g
    v_new = beta2 * v + (1 - beta2) * g * g
    t = step.to(theta.device).float()[:, None]
    mhat = m_new / (1 - beta1 ** t)
    vhat = v_new / (1 - beta2 ** t)
    new = theta - lr.to(theta.device).float()[:, None] * mhat / (vhat.sqrt() + eps)
    m.copy_(torch.where(a, m_new, m))
    v.copy_(torch.where(a, v_new, v))
    theta.copy_(torch.where(a, new, theta))
    if shadow is not None:
        shadow.copy_(theta.to(shadow.dtype))


def weighted_sum(x, w, out=None):
    """out (fp64) += Σ_k w_k x[k,:] accumulated in fp64 (reference FedAvg accumulates in
    float64: `fed_avg_algorithm.py:39-52`). Returns the fp64 [P] accumulator."""
    acc = (x.double() * w.double().to(x.device)[:, None]).sum(dim=0)
    if out is None:
        return acc
    return out.add_(acc)


TRIM_MAX_ROWS = 512  # csrc/dls.h


def trim_keys(x):
    """Signed int32 sort keys of fp32 values: bits ^ ((bits >> 31) & 0x7fffffff). Monotone over the
    non-NaN floats, −0 below +0, negative-sign NaNs below −inf, positive-sign NaNs above +inf; equal
    keys are equal bit patterns."""
    bits = x.contiguous().view(torch.int32)
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def check_trim(n: int, b: int) -> None:
    if not 1 <= n <= TRIM_MAX_ROWS:
        raise ValueError(f"trimmed_sum supports 1 to {TRIM_MAX_ROWS} rows, got {n}")
    if not 0 <= 2 * b < n:
        raise ValueError(f"trimmed_sum needs 0 <= 2b < n, got b={b}, n={n}")


def trimmed_sum(x, b, out=None):
    """Coordinate-wise trimmed sum (the oracle of csrc/robust.hip): per column of x [n, P] the values
    are sorted by `trim_keys`, the b lowest and b highest dropped and the other n − 2b added as
    doubles one at a time in ascending order from +0.0. A NaN sum is the canonical quiet NaN
    (0x7ff8000000000000). Returns fp64 [P] (written into out[:P] if given)."""
    n, P = x.shape
    check_trim(n, b)
    assert x.dtype == torch.float32
    order = torch.sort(trim_keys(x), dim=0).indices
    rows = torch.gather(x, 0, order)
    acc = torch.zeros(P, dtype=torch.float64, device=x.device)
    for r in range(b, n - b):
        acc = acc + rows[r].double()
    nan = torch.tensor(0x7FF8000000000000, dtype=torch.int64, device=x.device).view(torch.float64)
    acc = torch.where(acc.isnan(), nan, acc)
    if out is None:
        return acc
    assert out.dtype == torch.float64 and out.dim() == 1 and out.numel() >= P
    out[:P].copy_(acc)
    return out


PAIR_SPAN = 4096  # W: columns per span of pairwise_sq_dists (csrc/dls.h)
PAIR_GROUP = 8  # G: consecutive spans per group


def check_pairs(n: int) -> None:
    if not 1 <= n <= TRIM_MAX_ROWS:
        raise ValueError(f"pairwise_sq_dists supports 1 to {TRIM_MAX_ROWS} rows, got {n}")


def pairwise_sq_dists(x, out=None):
    """Squared L2 distances between the rows of x [n, P] fp32 (the oracle of csrc/krum.hip, and the
    CPU path): fp64 [n, n] (written into `out` if given).

    term(i, j, p) = fl64(d · d) with d = fl64(double(x[i, p]) − double(x[j, p])); the multiply and the
    add that follows are rounded separately (no FMA); denormal inputs are not flushed. D[i, j] adds
    the terms in an order fixed by the column index alone: the columns are cut into spans of W =
    PAIR_SPAN = 4096 columns (the last may be shorter) and the spans into groups of G = PAIR_GROUP = 8
    consecutive spans;
      span sum  = the span's terms added one at a time in ascending column order from +0.0,
      group sum = the group's span sums added in ascending span order from +0.0,
      D[i, j]   = the group sums added in ascending group order from +0.0.
    Nothing depends on n, the row order or the device: D[i, i] is +0.0 for a finite row, D[i, j] and
    D[j, i] have the same bits, a row permutation permutes D, zero columns change nothing, D is finite
    where both rows are, NaN / ±inf follow IEEE (NaN payload bits are not part of the contract).
    1 ≤ n ≤ 512, else ValueError.

    The loops below run over the position inside a span (all spans at once), then over the span
    inside a group, then over the groups: plain tensor adds, no `sum` / `cumsum`."""
    n, P = x.shape
    check_pairs(n)
    assert x.dtype == torch.float32
    W, G = PAIR_SPAN, PAIR_GROUP
    xd = x.double()
    full, tail = P // W, P % W
    sums = torch.zeros((full + (1 if tail else 0), n, n), dtype=torch.float64, device=x.device)  # per span
    d = torch.empty((max(full, 1), n, n), dtype=torch.float64, device=x.device)
    if full:
        cols = xd[:, : full * W].reshape(n, full, W).permute(2, 1, 0).contiguous()  # [W, span, row]
        acc = sums[:full]
        for c in range(W):
            torch.sub(cols[c][:, :, None], cols[c][:, None, :], out=d[:full])
            d[:full].mul_(d[:full])
            acc.add_(d[:full])
    if tail:
        cols = xd[:, full * W :].t().contiguous()  # [tail, row]
        acc = sums[full]
        for c in range(tail):
            torch.sub(cols[c][:, None], cols[c][None, :], out=d[0])
            d[0].mul_(d[0])
            acc.add_(d[0])
    res = torch.zeros((n, n), dtype=torch.float64, device=x.device)
    for g0 in range(0, sums.shape[0], G):
        group = torch.zeros((n, n), dtype=torch.float64, device=x.device)
        for s in range(g0, min(g0 + G, sums.shape[0])):
            group = group + sums[s]
        res = res + group
    if out is None:
        return res
    assert out.dtype == torch.float64 and out.shape == (n, n)
    out.copy_(res)
    return out


def row_sq_norms(x, out=None):
    """Squared L2 norm of every row of x [n, P] fp32 (the oracle of csrc/dp.hip row_sq_norms, and the
    CPU path): fp64 [n] (written into out[:n] if given).

    term(k, p) = fl64(double(x[k, p]) · double(x[k, p])) — exact, a 24-bit mantissa squared fits in 53
    bits — added in the order of `pairwise_sq_dists`: spans of W = PAIR_SPAN columns one term at a time
    in ascending column order from +0.0, groups of G = PAIR_GROUP span sums in ascending span order
    from +0.0, the group sums in ascending group order from +0.0. Denormals are not flushed; nothing
    depends on n. So row_sq_norms(x)[k] has the bits of pairwise_sq_dists(stack([x[k], zeros]))[0, 1].

    Like `pairwise_sq_dists`, the loops run over the position inside a span (all spans at once), the
    span inside a group, then the groups: plain tensor adds, no `sum` / `cumsum`."""
    n, P = x.shape
    assert x.dtype == torch.float32
    W, G = PAIR_SPAN, PAIR_GROUP
    xd = x.double()
    full, tail = P // W, P % W
    sums = torch.zeros((full + (1 if tail else 0), n), dtype=torch.float64, device=x.device)  # per span
    if full:
        cols = xd[:, : full * W].reshape(n, full, W).permute(2, 1, 0).contiguous()  # [W, span, row]
        acc = sums[:full]
        for c in range(W):
            acc.add_(cols[c] * cols[c])
    if tail:
        cols = xd[:, full * W :].t().contiguous()  # [tail, row]
        acc = sums[full]
        for c in range(tail):
            acc.add_(cols[c] * cols[c])
    res = torch.zeros(n, dtype=torch.float64, device=x.device)
    for g0 in range(0, sums.shape[0], G):
        group = torch.zeros(n, dtype=torch.float64, device=x.device)
        for s in range(g0, min(g0 + G, sums.shape[0])):
            group = group + sums[s]
        res = res + group
    if out is None:
        return res
    assert out.dtype == torch.float64 and out.dim() == 1 and out.numel() >= n
    out[:n].copy_(res)
    return out


def check_clip(clip) -> float:
    clip = float(clip)
    if not (clip > 0.0 and math.isfinite(clip)):
        raise ValueError(f"the clip norm must be a finite positive number, got {clip}")
    return clip


def clip_scales(nsq, clip):
    """(s fp64 [n], rejected bool [n]) of squared norms nsq fp64 [n]: norm = sqrt(nsq); s = clip / norm
    if norm > clip, else exactly 1.0; a non-finite nsq (NaN or ±inf in the row, or a finite row whose
    square sum overflows) gives s = 0 and rejected = True. sqrt, the comparison and the division are
    correctly rounded IEEE operations: the same bits on every backend. (Evaluated with python floats
    over the n values: `torch.sqrt` on the CPU is not correctly rounded in every build.)"""
    clip = check_clip(clip)
    assert nsq.dtype == torch.float64 and nsq.dim() == 1
    s, rejected = [], []
    for v in nsq.tolist():
        bad = not math.isfinite(v)
        norm = math.sqrt(v) if not bad and v >= 0.0 else float("nan")
        s.append(0.0 if bad else clip / norm if norm > clip else 1.0)
        rejected.append(bad)
    return (torch.tensor(s, dtype=torch.float64, device=nsq.device),
            torch.tensor(rejected, dtype=torch.bool, device=nsq.device))


def clipped_sum(x, nsq, clip, out=None):
    """out (fp64 [≥ P]; zeros [P] if None)[:P] += the rows of x [n, P] fp32 scaled by `clip_scales(nsq,
    clip)`: for k ascending, out[p] = fl64(out[p] + fl64(s_k · double(x[k, p]))), multiply and add
    rounded separately; rejected rows are skipped (0 · NaN would poison the sum). An unclipped row
    (s_k = 1.0) adds double(x) exactly. The oracle of csrc/dp.hip clipped_sum, and the CPU path."""
    n, P = x.shape
    assert x.dtype == torch.float32 and nsq.shape == (n,)
    s, rejected = clip_scales(nsq, clip)
    if out is None:
        out = torch.zeros(P, dtype=torch.float64, device=x.device)
    assert out.dtype == torch.float64 and out.dim() == 1 and out.numel() >= P
    acc = out[:P]
    s_host, rej_host = s.tolist(), rejected.tolist()
    for k in range(n):
        if rej_host[k]:
            continue
        acc.add_(x[k].double() * s_host[k])
    return out


PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57  # Random123 Philox4x32 multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85  # ... and Weyl key increments
DP_NOISE_TAG = 0x44503031  # fourth counter word of gaussian_add ("DP01")
_M32 = 0xFFFFFFFF


def _mulhilo32(m: int, a):
    """(high, low) 32-bit words of m · a for a 32-bit constant m and int64 tensors a < 2^32. The
    product exceeds 2^63, so it is formed from 16-bit halves (every partial sum stays below 2^34)."""
    mh, ml = m >> 16, m & 0xFFFF
    ah, al = a >> 16, a & 0xFFFF
    mid = ah * ml + al * mh
    low = al * ml + ((mid & 0xFFFF) << 16)
    return ah * mh + (mid >> 16) + (low >> 32), low & _M32


def philox4x32(counter, key, rounds: int = 10):
    """Philox4x32-`rounds` (Salmon et al. 2011; the Random123 constants). counter: four int64 tensors
    (or ints) holding 32-bit words, key: two ints. Returns the four output words as int64 tensors."""
    c0, c1, c2, c3 = (torch.as_tensor(c, dtype=torch.int64) & _M32 for c in counter)
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    for _ in range(rounds):
        hi0, lo0 = _mulhilo32(PHILOX_M0, c0)
        hi1, lo1 = _mulhilo32(PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def philox4x32_int(counter, key, rounds: int = 10) -> tuple[int, int, int, int]:
    """`philox4x32` for one counter of four python ints: the same words as python ints, without a tensor
    (the host-side protocol of secure aggregation draws thousands of single values a round)."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def gaussian_noise(P: int, seed: int, stream: int, start: int = 0, device=None):
    """fp64 [P] standard normal draws z[start], ..., z[start + P − 1] of the (seed, stream) sequence:
    for the pair index i = p // 2, Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
    (i & 0xffffffff, i >> 32, stream, 0x44503031) gives w0..w3,
      u1 = (((w0 >> 5) << 26) + (w1 >> 6) + 1) · 2^-53 in (0, 1],
      u2 = (((w2 >> 5) << 26) + (w3 >> 6)) · 2^-53 in [0, 1),
      r = sqrt(−2 · log(u1)), φ = fl64(2π · u2), z[2i] = r · cos φ, z[2i + 1] = r · sin φ  (Box-Muller),
    all in fp64. z[p] depends on (seed, stream, p) only."""
    seed, stream = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & _M32
    first, last = start // 2, (start + P + 1) // 2
    i = torch.arange(first, max(last, first), dtype=torch.int64, device=device)
    w0, w1, w2, w3 = philox4x32((i & _M32, i >> 32, torch.full_like(i, stream), torch.full_like(i, DP_NOISE_TAG)),
                                (seed & _M32, seed >> 32))
    u1 = (((w0 >> 5) << 26) + (w1 >> 6) + 1).double() * 2.0 ** -53
    u2 = (((w2 >> 5) << 26) + (w3 >> 6)).double() * 2.0 ** -53
    r = torch.sqrt(-2.0 * torch.log(u1))
    phi = (2.0 * math.pi) * u2
    z = torch.stack([r * torch.cos(phi), r * torch.sin(phi)], dim=1).reshape(-1)
    return z[start - 2 * first : start - 2 * first + P]


def gaussian_add(acc, std, seed, stream, mask=None):
    """acc (fp64 [P]) [p] += fl64(std · z[p]) wherever mask[p] != 0 (`mask` None: everywhere), z =
    `gaussian_noise(P, seed, stream)`. Masked-out elements are not written. Returns `acc`."""
    assert acc.dtype == torch.float64 and acc.dim() == 1
    P = acc.numel()
    t = gaussian_noise(P, seed, stream, device=acc.device) * float(std)
    if mask is None:
        return acc.add_(t)
    assert mask.shape == (P,)
    m = mask != 0
    acc[m] = acc[m] + t[m]
    return acc


# ------------------------------------------------------------------ pairwise-masked secure aggregation
SECAGG_TAG = 0x53413031  # fourth counter word of the mask streams ("SA01")
SECAGG_MAX_ROWS = 512  # csrc/dls.h
_SECAGG_CHUNK = 1 << 20  # Philox calls per vectorised step of the oracle


def secagg_frac_bits(R, m: int, f=None) -> tuple[float, int]:
    """(R as the fp32 value the clamp uses, f) of the fixed-point code of `secagg_mask_rows`. R must be a
    finite number > 0 (it is rounded to fp32 once, and the bound below uses the rounded value); m ≥ 1 is the
    fixed cohort size. f = `f` if given, else the largest integer with m · R · 2^f ≤ 2^31 − 1, so that the sum
    of m codes cannot wrap. ValueError if a given f breaks that bound or is below 1, or if the computed f is
    below 1."""
    from fractions import Fraction

    try:
        R = float(R)
    except (TypeError, ValueError) as e:
        raise ValueError(f"secagg: the range must be a number ({e})") from e
    if not (R > 0.0 and math.isfinite(R)):
        raise ValueError(f"secagg: the range must be a finite positive number, got {R}")
    R = float(torch.tensor(R, dtype=torch.float32))
    m = int(m)
    if not (R > 0.0 and math.isfinite(R)) or m < 1:
        raise ValueError(f"secagg: range {R} (as fp32) and cohort size {m} must be positive and finite")
    room = Fraction(2 ** 31 - 1) / (Fraction(R) * m)
    if f is None:
        f = 0
        while Fraction(2) ** (f + 1) <= room:
            f += 1
        if f < 1:
            raise ValueError(f"secagg: no fixed-point code with >= 1 fractional bit fits m = {m}, R = {R} in 2^31")
        return R, f
    if isinstance(f, bool) or int(f) != f:
        raise ValueError(f"secagg: frac_bits must be an integer, got {f!r}")
    f = int(f)
    if f < 1 or Fraction(2) ** f > room:
        raise ValueError(f"secagg: frac_bits = {f} overflows the ring: m * R * 2^f must stay <= 2^31 - 1 "
                         f"(m = {m}, R = {R}) with f >= 1")
    return R, f


def _philox_keys(i, k0, k1):
    """Philox4x32-10 with counter (i lo, i hi, 0, SECAGG_TAG) for int64 tensors i, k0, k1 that broadcast."""
    c0, c1, c2, c3 = i & _M32, i >> 32, torch.zeros_like(i), torch.full_like(i, SECAGG_TAG)
    for _ in range(10):
        hi0, lo0 = _mulhilo32(PHILOX_M0, c0)
        hi1, lo1 = _mulhilo32(PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return c0, c1, c2, c3


def secagg_mask_words(key: int, P: int, start: int = 0, device=None):
    """int64 [P] holding the unsigned 32-bit mask words w(κ, p), p = start .. start + P − 1: word p % 4 of
    Philox4x32-10 with key (κ & 0xffffffff, κ >> 32) and counter (i & 0xffffffff, i >> 32, 0, 0x53413031), i =
    p // 4. w depends on (κ, p) alone."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    first, last = start // 4, (start + P + 3) // 4
    i = torch.arange(first, max(last, first), dtype=torch.int64, device=device)
    k0 = torch.full_like(i, key & _M32)
    w = torch.stack(_philox_keys(i, k0, torch.full_like(i, key >> 32)), dim=1).reshape(-1)
    return w[start - 4 * first : start - 4 * first + P]


def check_secagg_entries(keys, signs) -> tuple[list[int], list[int]]:
    keys, signs = [int(k) for k in keys], [int(s) for s in signs]
    if len(keys) != len(signs):
        raise ValueError(f"secagg: {len(keys)} keys for {len(signs)} signs")
    if any(s not in (1, -1) for s in signs):
        raise ValueError("secagg: every sign is +1 or -1")
    if any(not 0 <= k < 2 ** 64 for k in keys):
        raise ValueError("secagg: every key is an unsigned 64-bit integer")
    return keys, signs


def secagg_mask_sum(keys, signs, P: int, device=None):
    """int64 [P]: Σ_e signs[e] · w(keys[e], p) as an exact signed sum (|·| < 2^32 · len(keys))."""
    keys, signs = check_secagg_entries(keys, signs)
    assert P % 4 == 0
    n4 = P // 4
    total = torch.zeros(P, dtype=torch.int64, device=device)
    if not keys or not P:
        return total
    i = torch.arange(n4, dtype=torch.int64, device=device)[None, :]
    step = max(1, _SECAGG_CHUNK // n4)
    for e0 in range(0, len(keys), step):
        ks = keys[e0 : e0 + step]
        k0 = torch.tensor([k & _M32 for k in ks], dtype=torch.int64, device=device)[:, None]
        k1 = torch.tensor([k >> 32 for k in ks], dtype=torch.int64, device=device)[:, None]
        sg = torch.tensor(signs[e0 : e0 + step], dtype=torch.int64, device=device)[:, None, None]
        w = torch.stack(_philox_keys(i, k0, k1), dim=2)  # [entries, P / 4, 4]
        total += (w * sg).sum(0).reshape(-1)
    return total


def secagg_quantise(x, R: float, f: int):
    """(q int64 [K, P], stats int32 [K, 2]) of fp32 rows x: t = x clamped to [−R, R] in fp32 (±inf clamp to
    ±R), q = rint(fl64(t) · 2^f) with ties to even — the scaling is exact in fp64, so this is the only
    rounding — and q = 0 for a NaN. stats[k] = (elements with |x| > R, infinities included; NaN elements)."""
    assert x.dtype == torch.float32 and x.dim() == 2
    nan = torch.isnan(x)
    t = torch.clamp(torch.where(nan, torch.zeros_like(x), x), min=-R, max=R)
    q = torch.round(t.double() * float(2 ** f)).to(torch.int64)
    stats = torch.stack([(x.abs() > R).sum(1), nan.sum(1)], dim=1).to(torch.int32)
    return q, stats


def check_secagg_rows(x, out, offsets, keys, signs):
    """(K, P, offsets, keys, signs) of the operands of `secagg_mask_rows`; ValueError on a wrong dtype,
    shape, stride, alignment, entry table or row count (both backends call this before they touch anything)."""
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("secagg_mask_rows: x must be fp32 [K, P] with unit column stride")
    K, P = x.shape
    if not 1 <= K <= SECAGG_MAX_ROWS:
        raise ValueError(f"secagg_mask_rows supports 1 to {SECAGG_MAX_ROWS} rows, got {K}")
    if P % 4:
        raise ValueError(f"secagg_mask_rows: P must be a multiple of 4, got {P}")
    for name, t in (("x", x), ("out", out)):
        if t is None:
            continue
        if name == "out" and (t.dtype != torch.int32 or t.shape != (K, P) or (P > 1 and t.stride(1) != 1)
                              or t.device != x.device):
            raise ValueError(f"secagg_mask_rows: out must be int32 [{K}, {P}] with unit column stride on x's device")
        if t.data_ptr() % 16 or (K > 1 and (t.stride(0) % 4 or t.stride(0) < P)):
            raise ValueError(f"secagg_mask_rows: the rows of {name} must be 16-B aligned and must not overlap")
    if out is not None and out.data_ptr() == x.data_ptr() and K > 1 and out.stride(0) != x.stride(0):
        raise ValueError("secagg_mask_rows: an in-place out must have x's row stride")
    offsets = [int(o) for o in offsets]
    keys, signs = check_secagg_entries(keys, signs)
    if len(offsets) != K + 1 or offsets[0] != 0 or offsets[-1] != len(keys) or any(
            a > b for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"secagg_mask_rows: offsets must be {K + 1} ascending entry indices from 0 to {len(keys)}")
    if any(b - a > SECAGG_MAX_ROWS for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"secagg_mask_rows: at most {SECAGG_MAX_ROWS} entries per row")
    return K, P, offsets, keys, signs


def _to_int32(v):
    """The low 32 bits of int64 values as signed int32."""
    v = v & _M32
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def secagg_mask_rows(x, offsets, keys, signs, R, f, out=None):
    """The masked upload (`ops.fl.secagg_mask_rows` states the contract; the oracle of csrc/secagg.hip and the
    CPU path): (out int32 [K, P], stats int32 [K, 2]) with out[k, p] = the low 32 bits of q(x[k, p]) + Σ_e
    sign_e · w(κ_e, p) over the entries offsets[k] .. offsets[k + 1] − 1 of row k. `out` may alias x."""
    K, P, offsets, keys, signs = check_secagg_rows(x, out, offsets, keys, signs)
    R, f = secagg_frac_bits(R, 1, f)
    q, stats = secagg_quantise(x, R, f)
    for k in range(K):
        a, b = offsets[k], offsets[k + 1]
        q[k] += secagg_mask_sum(keys[a:b], signs[a:b], P, device=x.device)
    res = _to_int32(q)
    if out is None:
        return res, stats
    out.copy_(res)
    return out, stats


def check_ring_operands(acc, rows=None) -> int:
    if acc.dtype != torch.int64 or acc.dim() != 1 or not acc.is_contiguous() or acc.data_ptr() % 16:
        raise ValueError("ring: acc must be a contiguous, 16-B aligned int64 vector")
    P = acc.numel()
    if P % 4:
        raise ValueError(f"ring: P must be a multiple of 4, got {P}")
    if rows is not None:
        if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != P or (P > 1 and rows.stride(1) != 1):
            raise ValueError(f"ring_sum: rows must be int32 [K, {P}] with unit column stride")
        K = rows.shape[0]
        if not 1 <= K <= SECAGG_MAX_ROWS:
            raise ValueError(f"ring_sum supports 1 to {SECAGG_MAX_ROWS} rows, got {K}")
        if rows.device != acc.device or rows.data_ptr() % 16 or (K > 1 and (rows.stride(0) % 4 or rows.stride(0) < P)):
            raise ValueError("ring_sum: rows must be on acc's device, 16-B aligned and must not overlap")
    return P


def ring_sum(rows, acc):
    """acc (int64 [P]) [p] += Σ_k (int64) rows[k, p] (sign-extended int32 rows, ≤ 512 of them: no int64
    overflow; the low 32 bits are the sum in Z_{2^32}). Returns `acc`."""
    check_ring_operands(acc, rows)
    return acc.add_(rows.to(torch.int64).sum(0))


def ring_unmask(acc, keys, signs):
    """acc (int64 [P]) [p] −= Σ_e signs[e] · (int64) w(keys[e], p) over one flat entry list (≤ 512 · 512
    entries: no overflow). Returns `acc`."""
    P = check_ring_operands(acc)
    keys, signs = check_secagg_entries(keys, signs)
    if len(keys) > SECAGG_MAX_ROWS * SECAGG_MAX_ROWS:
        raise ValueError(f"ring_unmask: at most {SECAGG_MAX_ROWS * SECAGG_MAX_ROWS} entries, got {len(keys)}")
    return acc.sub_(secagg_mask_sum(keys, signs, P, device=acc.device))


def ring_decode(acc, f: int):
    """fp64 [P]: v · 2^−f with v = the low 32 bits of acc[p] as a signed int32 (exact)."""
    assert acc.dtype == torch.int64
    return _to_int32(acc).to(torch.float64) * (2.0 ** -int(f))


SERVER_OPT_RULES = ("sgdm", "adagrad", "adam", "yogi")  # the kernel's rule index is the position here


def check_server_opt(rule, lr, beta1, beta2, tau) -> tuple[str, float, float, float, float]:
    """(rule, lr, β1, β2, τ) of `server_opt_step` as a rule name and python floats; ValueError on a rule
    that does not exist, a non-finite number, β outside [0, 1) or, for the adaptive rules, τ ≤ 0."""
    if rule not in SERVER_OPT_RULES:
        raise ValueError(f"server_opt_step: unknown rule {rule!r}; one of {SERVER_OPT_RULES}")
    try:
        lr, beta1, beta2, tau = float(lr), float(beta1), float(beta2), float(tau)
    except (TypeError, ValueError) as e:
        raise ValueError(f"server_opt_step: lr, beta1, beta2 and tau must be numbers ({e})") from e
    if not math.isfinite(lr):
        raise ValueError(f"server_opt_step: lr must be finite, got {lr}")
    for name, b in (("beta1", beta1), ("beta2", beta2)):
        if not 0.0 <= b < 1.0:  # (false for NaN too)
            raise ValueError(f"server_opt_step: {name} must lie in [0, 1), got {b}")
    if not math.isfinite(tau) or (rule != "sgdm" and not tau > 0.0):
        raise ValueError(f"server_opt_step: tau must be finite and, for the adaptive rules, positive; got {tau}")
    return rule, lr, beta1, beta2, tau


def check_server_opt_operands(theta, target, m, v, rule, x_out=None) -> int:
    """P of the operands of `server_opt_step`; ValueError on a wrong dtype, shape, stride or alignment
    (both backends call this before they touch anything)."""
    if theta.dtype != torch.float32 or theta.dim() != 1 or not theta.is_contiguous():
        raise ValueError("server_opt_step: theta must be a contiguous fp32 vector")
    P = theta.numel()
    if P % 4:
        raise ValueError(f"server_opt_step: P must be a multiple of 4, got {P}")
    if theta.data_ptr() % 16:
        raise ValueError("server_opt_step: theta must be 16-B aligned")
    if (v is None) != (rule == "sgdm"):
        raise ValueError("server_opt_step: v is None for sgdm and an fp64 [P] tensor for the adaptive rules")
    for name, t, exact in (("target", target, False), ("m", m, True), ("v", v, True), ("x_out", x_out, True)):
        if t is None and name in ("v", "x_out"):
            continue
        if t is None or t.dtype != torch.float64 or t.dim() != 1 or not t.is_contiguous() or t.device != theta.device:
            raise ValueError(f"server_opt_step: {name} must be a contiguous fp64 vector on theta's device")
        if t.numel() != P if exact else t.numel() < P:
            raise ValueError(f"server_opt_step: {name} has {t.numel()} elements for P = {P}")
        if t.data_ptr() % 32:
            raise ValueError(f"server_opt_step: {name} must be 32-B aligned")
    return P


def server_opt_step(theta, target, m, v, rule, lr, beta1, beta2, tau, c1, c2, x_out=None):
    """One server optimiser step on the pseudo-gradient d = target − θ (`ops.fl.server_opt_step` states
    the contract): θ fp32 [P], m and v fp64 [P] are updated in place, `target` fp64 [≥ P] is read-only,
    the pre-cast fp64 x goes to `x_out` if given. Every line below is one fp64 operation rounded once;
    sqrt is numpy's (correctly rounded; the CPU `torch.sqrt` is not in every build), and so is the cast
    to fp32 (round to nearest even, overflow to ±inf). The oracle of csrc/server_opt.hip and the CPU
    path. c1 = 1 − β1 and c2 = 1 − β2 come from the caller, who forms them once for both backends."""
    import numpy as np

    rule, lr, beta1, beta2, tau = check_server_opt(rule, lr, beta1, beta2, tau)
    P = check_server_opt_operands(theta, target, m, v, rule, x_out)
    if P == 0:
        return theta
    if theta.device.type != "cpu":  # (the forced torch backend on a device: step on the host, copy back)
        dev = [theta, m, v, x_out]
        host = [None if t is None else t.cpu() for t in dev]
        server_opt_step(host[0], target[:P].cpu(), host[1], host[2], rule, lr, beta1, beta2, tau, c1, c2, host[3])
        for t, h in zip(dev, host):
            if t is not None:
                t.copy_(h)
        return theta
    c1, c2 = float(c1), float(c2)
    with np.errstate(all="ignore"):
        th32 = theta.numpy()  # (shares memory: the in-place writes below reach the tensors)
        th = th32.astype(np.float64)
        t = target[:P].numpy()
        mm = m.numpy()
        d = t - th
        ok = np.isfinite(d)
        q = d * d
        m1 = beta1 * mm
        if rule == "sgdm":
            m1 = m1 + d
        else:
            g1 = c1 * d
            m1 = m1 + g1
            vv = v.numpy()
            if rule == "adagrad":
                v1 = vv + q
            elif rule == "adam":
                v1 = beta2 * vv
                g2 = c2 * q
                v1 = v1 + g2
            else:
                g2 = c2 * q
                z = vv - q
                sign = (z > 0.0).astype(np.float64) - (z < 0.0).astype(np.float64)  # (0 for z == 0 and NaN)
                g2 = g2 * sign
                v1 = vv - g2
        step = lr * m1
        if rule != "sgdm":
            den = np.sqrt(v1)
            den = den + tau
            step = step / den
        x = th + step
        x = np.where(ok, x, t)  # a non-finite d: θ' = fl32(target), the state keeps its bits
        if x_out is not None:
            x_out.numpy()[...] = x
        th32[...] = x.astype(np.float32)
        np.copyto(mm, m1, where=ok)
        if rule != "sgdm":
            np.copyto(vv, v1, where=ok)
    return theta


def krum_scores(D, f: int):
    """(scores [n] fp64, f actually used): the Krum score of row i is the sum of its k = clamp(n − f −
    2, 1, n − 1) smallest D[i, j], j ≠ i, added in ascending order in fp64 from +0.0; a non-finite
    distance counts as +inf; n = 1 scores 0. If n < 2f + 3 (a round shrunk by failures) f is replaced
    by max(0, (n − 3) // 2), with a warning."""
    D = D.detach().to("cpu", torch.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    f = max(0, int(f))
    if n < 2 * f + 3:
        from ..utils.logging import get_logger

        f2 = max(0, (n - 3) // 2)
        if f2 != f:
            get_logger().warning("krum: %d uploads cannot carry f = %d (needs n >= 2f + 3): using f = %d", n, f, f2)
        f = f2
    if n == 1:
        return torch.zeros(1, dtype=torch.float64), f
    k = min(max(n - f - 2, 1), n - 1)
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    d = torch.where(torch.isfinite(D), D, inf)
    off = d[~torch.eye(n, dtype=torch.bool)].reshape(n, n - 1)  # row i without D[i, i]
    srt = torch.sort(off, dim=1).values
    scores = torch.zeros(n, dtype=torch.float64)
    for c in range(k):
        scores = scores + srt[:, c]
    return scores, f


def krum_select(D, f: int, m: int, ids) -> list:
    """Row indices of the m uploads with the smallest (Krum score, client id), sorted by client id.
    `ids[i]` is the client id of row i (the tie-break, so the choice does not depend on which rank or
    wave hosts a client); m is clamped to [1, n]. Scores: `krum_scores`. Runs on the host for both
    backends, so a bitwise-equal D gives an identical selection."""
    scores, _ = krum_scores(D, f)
    n = scores.numel()
    ids = [int(c) for c in ids]
    assert len(ids) == n and len(set(ids)) == n, "one distinct client id per row"
    m = min(max(int(m), 1), n)
    sc = scores.tolist()
    order = sorted(range(n), key=lambda i: (sc[i], ids[i]))[:m]
    return sorted(order, key=lambda i: ids[i])


def mix_rows(x, w, out_dtype=torch.float32):
    """Subset models W[M, K] · x[K, P] (fp64 accumulation), cast to `out_dtype`."""
    return (w.double().to(x.device) @ x.double()).to(out_dtype)


def masked_weighted_sum(x, mask, w, num=None, den=None):
    """FedDropoutAvg: numerator Σ w_k m_k x_k and per-element denominator Σ w_k m_k (fp64)."""
    wm = mask.double() * w.double().to(x.device)[:, None]
    n, d = (x.double() * wm).sum(0), wm.sum(0)
    if num is not None:
        n = num.add_(n)
        d = den.add_(d)
    return n, d


def broadcast_rows(dst, src, rows=None):
    if rows is None:
        dst.copy_(src.unsqueeze(0).expand_as(dst))
    else:
        dst[rows] = src.unsqueeze(0).to(dst.dtype)


def delta(theta, base):
    return theta - base.unsqueeze(0)


def split_rows(theta, split):
    """split[k] = (bf16 hi, bf16 lo) planes of theta[k]: hi = RNE(x), lo = RNE(x - hi)."""
    hi = theta.to(torch.bfloat16)
    split[:, 0].copy_(hi)
    split[:, 1].copy_((theta - hi.float()).to(torch.bfloat16))
