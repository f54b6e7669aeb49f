"""Shared by tests/test_attention_oracle.py, tests/test_attention_edges_gpu.py and tests/test_spmm_gpu.py:
float64 oracles of attention (forward, backward, key padding, probability dropout) and SpMM, the
input builders of those files, the error metric of tests/test_kernels_f32_gpu.py and the bounds of
the existing attention / SpMM tests, named once.

Everything here runs on the CPU in float64 and is written out plainly: scores, mask, softmax, the
optional dropout factor, matmuls. `ops.ref.attn_fwd` / `attn_bwd` cast their arguments to fp32, so
they are the fp32 CPU path under test in test_attention_oracle.py, not the oracle.

The kv = 0 contract (a sequence without a valid key: `data/datasets.py` clamps lengths only from
above, an empty text reaches the model): o = 0, lse = 0, dq = dk = dv = 0, exactly. The kernels
compute this on purpose (`l > 0 ? … : 0`); the oracle states it as a branch of its own.
"""

import contextlib
import math

import torch

# ---- bounds (max |out − exact| / max |exact|), all taken from tests that predate this file; none was
# derived from what the kernels under test produce
F32_TOL = 3e-5  # fp32 o: test_attention_mfma / test_attention_embedding_f32
BF16_MFMA_TOL = 2.5e-2  # bf16 o on the MFMA kernels: test_attention_mfma
BF16_VALU_TOL = 2e-2  # bf16 o on the VALU kernels: test_attention_fwd_bwd ...
BF16_VALU_GRAD_TOL = 3e-2  # ... and its gradients
REF_TOL = 1e-5  # fp32 ops.ref against float64 (tests/test_kernels_f32_gpu.py TOL)
SPMM_F32_TOL = 1e-5
SPMM_BF16_TOL = 2e-2  # test_spmm_shared_and_flat


def lse_tol(tol: float) -> float:
    """lse is held to the forward bound, and to no less than 1e-5 (test_attention_mfma)."""
    return max(tol, 1e-5)


def tols(dtype, valu: bool = False) -> tuple[float, float]:
    """(forward, gradient) bound of a kernel path: gradients get twice the forward bound, except the
    bf16 VALU pair which test_attention_fwd_bwd states."""
    if dtype == torch.float32:
        return F32_TOL, 2 * F32_TOL
    if valu:
        return BF16_VALU_TOL, BF16_VALU_GRAD_TOL
    return BF16_MFMA_TOL, 2 * BF16_MFMA_TOL


def d(t):
    return t.detach().cpu().double()


def rel_err(out, exact) -> float:
    """max |out − exact| / max |exact| on CPU doubles (the scale of the output), `_close` of
    tests/test_kernels_f32_gpu.py."""
    out, exact = d(out), d(exact)
    assert out.shape == exact.shape, (out.shape, exact.shape)
    assert torch.isfinite(out).all(), "non-finite output"
    return (out - exact).abs().max().item() / (exact.abs().max().item() + 1e-12)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------ oracles
def _masks(kv, K, B, L):
    """(valid keys [K,B,1,1,L] bool, empty sequences [K,B] bool) of key_valid [K,B] or None."""
    if kv is None:
        return torch.ones(K, B, 1, 1, L, dtype=torch.bool), torch.zeros(K, B, dtype=torch.bool)
    n = kv.detach().cpu().long().reshape(K, B)
    valid = torch.arange(L)[None, None, :] < n[..., None]
    return valid[:, :, None, None, :], n <= 0


def _softmax64(q, k, valid, empty):
    """(p [K,B,H,L,L], lse [K,B,H,L]) of the masked, scaled scores; an empty sequence is given one
    all-valid row of scores here (so nothing is NaN) and overwritten by the callers' kv = 0 branch."""
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill(~(valid | empty[:, :, None, None, None]), float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    return e / l, (m + torch.log(l)).squeeze(-1)


def attn_fwd64(q, k, v, kv=None, drop=None):
    """float64 attention over [K,B,H,L,dh]: (o, lse). kv [K,B] valid keys or None; drop the
    [K,B,H,L,L] factor M/(1−p) of `ref.attn_drop_scale` or None. lse is of the undropped scores."""
    q, k, v = d(q), d(k), d(v)
    K, B, H, L, _ = q.shape
    valid, empty = _masks(kv, K, B, L)
    p, lse = _softmax64(q, k, valid, empty)
    if drop is not None:
        p = p * d(drop)
    o = torch.matmul(p, v)
    if empty.any():  # kv = 0: no key to attend to
        o[empty] = 0.0
        lse[empty] = 0.0
    return o, lse


def attn_bwd64(do, q, k, v, kv=None, drop=None):
    """float64 (dq, dk, dv) from the oracle's own float64 o and lse."""
    do, q, k, v = d(do), d(q), d(k), d(v)
    K, B, H, L, dh = q.shape
    scale = 1.0 / math.sqrt(dh)
    valid, empty = _masks(kv, K, B, L)
    p, _ = _softmax64(q, k, valid, empty)
    fac = d(drop) if drop is not None else None
    pd = p * fac if fac is not None else p
    o = torch.matmul(pd, v)
    dv = torch.matmul(pd.transpose(-1, -2), do)
    dp = torch.matmul(do, v.transpose(-1, -2))
    if fac is not None:
        dp = dp * fac
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, k)
    dk = torch.matmul(ds.transpose(-1, -2), q)
    if empty.any():  # kv = 0: nothing depends on q, k or v
        for g in (dq, dk, dv):
            g[empty] = 0.0
    return dq, dk, dv


def drop_factor(shape, seeds, p: float):
    """The [K,B,H,L,L] dropout factor of `ref.attn_drop_scale` on the CPU (an integer hash of the
    client's seed, the head, the query and the key: reusable), or None for p = 0."""
    if not p:
        return None
    from distributed_learning_simulator_amd.ops import ref

    return ref.attn_drop_scale(shape, seeds.cpu(), p, "cpu")


def spmm64(rowptr, col, val, x):
    """float64 CSR [N, Nx] (one graph for all clients) times x [K, Nx, F] → [K, N, F], by index_add_."""
    rowptr, col = rowptr.detach().cpu().long(), col.detach().cpu().long()
    N = rowptr.numel() - 1
    x = d(x)
    rows = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1])
    y = torch.zeros(x.shape[0], N, x.shape[2], dtype=torch.float64)
    return y.index_add_(1, rows, x[:, col] * d(val)[None, :, None])


# ------------------------------------------------------------------------ inputs
def smooth(K, B, H, L, dh, seed=0, dtype=torch.float32):
    """randn q, k, v, do [K,B,H,L,dh] (CPU, already rounded to `dtype`): flat score distributions."""
    g = _gen(seed)
    return tuple(torch.randn(K, B, H, L, dh, generator=g).to(dtype) for _ in range(4))


def peaked(K, B, H, L, dh, spike_block, seed=0, dtype=torch.float32):
    """q, k, v, do with one dominant key per query inside the 32-key block `spike_block`.

    q = 4·randint(−2, 3), k = randint(−2, 3), v and do = randint(−8, 9) / 8: all exact in bf16. The
    block's keys j get sign patterns σ_j ∈ {±1}^dh, and every even query i is paired with the key j(i) =
    block start + i mod (keys in the block): q_i = |q_i|·σ_j(i), so k_j(i) = σ_j(i) = sign(q_i) wherever
    q_i ≠ 0 and that key scores Σ|q_i| / √dh ≈ 4.8·√dh (19 at dh 16, 38 at dh 64) against a standard
    deviation of 8 for the other keys. With dh ∈ {16, 64} the scale is a power of two and every score is
    an integer multiple of it below 2⁸: QKᵀ is exact in bf16, split-bf16 and fp32 alike. What rounding is
    left is in exp, in P (2⁻⁹ relative in bf16, ≤ 2⁻¹⁶ after the hi + lo split) and in the fp32 sums,
    which is why the bounds of the smooth inputs hold here unchanged.

    The odd queries keep their random signs on purpose. A row whose softmax is saturated has dS = P∘(dP −
    δ) ≈ 0 by cancellation of two O(1) numbers (dP of the dominant key and δ = dO·O): its true gradient
    is tiny, and the rounding of O alone — fp32 in `ops.ref`, bf16 in the bf16 kernels — leaves an
    absolute error in it of that rounding times |δ|, whatever the code does. With every row saturated
    max |exact| of dq and dk is itself that small and the metric measures only this cancellation (fp32
    `ops.ref` then shows 5e-5 for dq and 1.4e-4 for dk at dh 64); the unsaturated rows give the gradients
    their ordinary scale, as a real batch does, and the bounds apply to the whole tensor as usual."""
    g = _gen(seed)
    shape = (K, B, H, L, dh)
    q = 4 * torch.randint(-2, 3, shape, generator=g)
    qa = q.abs()
    k = torch.randint(-2, 3, shape, generator=g)
    v = torch.randint(-8, 9, shape, generator=g) / 8.0
    do = torch.randint(-8, 9, shape, generator=g) / 8.0
    j0 = spike_block * 32
    nb = min(32, L - j0)
    assert nb >= 1, (L, spike_block)
    sigma = torch.randint(0, 2, (K, B, H, nb, dh), generator=g) * 2 - 1
    k[:, :, :, j0 : j0 + nb] = sigma
    q = torch.where((torch.arange(L) % 2 == 0)[:, None], qa * sigma[:, :, :, torch.arange(L) % nb], q)
    out = tuple(t.to(torch.float32).to(dtype) for t in (q, k, v, do))
    for a, b in zip(out, (q, k, v, do)):
        assert torch.equal(a.double(), b.double())  # exact in `dtype`
    return out


def heads(t, H):
    """[K,B,L,D] → [K,B,H,L,dh] (a view)."""
    K, B, L, D = t.shape
    return t.reshape(K, B, L, H, D // H).permute(0, 1, 3, 2, 4)


def flat(t):
    """[K,B,H,L,dh] → [K,B,L,D]."""
    K, B, H, L, dh = t.shape
    return t.permute(0, 1, 3, 2, 4).reshape(K, B, L, H * dh)


# ------------------------------------------------------------------------ comparison
def check_attention(got, exact, kv, tol, gtol, what, cancel_scale=None):
    """got = (o, lse, dq, dk, dv) of the code under test, exact = the oracle's, all [K,B,H,L,·]. Every
    element is compared: the sequences with a valid key by `rel_err` against `tol` (o), `lse_tol(tol)`
    and `gtol` (gradients), the kv = 0 sequences with exact zeros; padded keys get exactly zero dk / dv.
    `cancel_scale` {name: scale}: a floor under max |exact| for outputs that are exactly 0 by cancellation
    (the caller says of what). Prints each figure before it asserts; returns {name: rel err}."""
    names = ("o", "lse", "dq", "dk", "dv")
    bounds = (tol, lse_tol(tol), gtol, gtol, gtol)
    K, B = got[0].shape[:2]
    n = None if kv is None else kv.detach().cpu().long().reshape(K, B)
    live = torch.ones(K, B, dtype=torch.bool) if n is None else n > 0
    errs = {}
    for name, g, e in zip(names, got, exact):
        g = d(g)
        assert torch.isfinite(g).all(), f"{what}: non-finite {name}"
        errs[name] = rel_err(g[live], e[live])
        if cancel_scale and name in cancel_scale:
            floor = max(e[live].abs().max().item(), cancel_scale[name])
            errs[name] = (g[live] - e[live]).abs().max().item() / floor
    print(f"ATTN_ERR {what} " + " ".join(f"{k}={v:.3g}/{b:.3g}" for (k, v), b in zip(errs.items(), bounds)))
    for (name, err), bound in zip(errs.items(), bounds):
        assert err <= bound, f"{what}: {name} rel err {err:.3g} > {bound}"
    for name, g in zip(names, got):
        assert torch.all(d(g)[~live] == 0), f"{what}: {name} of a kv = 0 sequence is not exactly 0"
    if n is not None:
        L = got[3].shape[-2]
        pad = torch.arange(L)[None, None, :] >= n[..., None]  # [K,B,L]
        for name, g in (("dk", got[3]), ("dv", got[4])):
            gz = d(g).permute(0, 1, 3, 2, 4)[pad]
            assert torch.all(gz == 0), f"{what}: {name} of a padded key is not exactly 0"
    return errs


@contextlib.contextmanager
def attn_mfma_option(hip, value):
    """Run a block with the native `attn_mfma` option set (0: the VALU fallback kernels), then put it
    back to the unset sentinel of options.py (the environment / kernel default), not to 1."""
    from distributed_learning_simulator_amd import options

    hip._C.set_native_option("attn_mfma", int(value))
    try:
        yield
    finally:
        hip._C.set_native_option("attn_mfma", options._NATIVE_UNSET)
