"""The attention kernels against the float64 oracle of tests/attention_common.py where they change
path: the VALU fallback kernels (csrc/attention.hip, `attn_mfma: 0`), which no other test runs; head
dim 48 on the MFMA kernels (the only one with a partly filled second 32-column tile); key counts and
sequence lengths on and beside the 32-key blocks and 128-row workgroups; a sequence without a valid
key; peaked score distributions (online-softmax rescale far from 1, probabilities that underflow);
dropout on the unpacked layout; and the support predicates against what the launchers do.

Every case runs forward and backward in fp32 and bf16 against the oracle on the upcast inputs, with
the bounds of the older attention tests (attention_common.py names them). Every element is compared;
the kv = 0 sequences are compared with exact zeros. The oracle of a case is computed once and shared
by the tests that use it.

What these tests found and the kernels now do (csrc/attention_mfma.hip, fp32 only): dk of a sequence
with ONE valid key beside 129-130 queries. There P = 1, o = v, and dS = P∘(dP − δ) is exactly 0 as the
difference of dP = dO·vᵀ (split-bf16 MFMA: operands cut to 16 mantissa bits, the lo·lo term dropped)
and δ = dO·o, which was an fp32 dot: 2⁻¹⁸·|dO||v| per column was left, and dK of that one key added it
over all L queries: |dk − 0| of 1.57e-4 (L 129, dh 32), 1.71e-4 (L 130, dh 48), 2.34e-4 (L 130, dh 64,
dropout 0.1) against max |dk| of 1.4-2.6 in the batch, i.e. 6.2e-5 to 1.0e-4 against the 6e-5 bound in
test_key_count_edges[mfma-32-fp32], test_unpacked_dropout[130-64-fp32] and test_head_dim_48[*-130-*-
fp32]. δ is now formed from the same split products as dP, and the dropout factor 1/(1−p) multiplies O,
dV and dP outside the products, so the two cancel to fp32 rounding: the same cases measure 8.2e-6 to
1.3e-5."""

import functools

import pytest
import torch

import attention_common as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, B, H = 2, 3, 2
SEEDS = torch.tensor([5, -9], dtype=torch.int32)
DTYPES = [torch.float32, torch.bfloat16]
KV_EDGE = ((1, 32, 33), (128, 129, 0))  # at L = 129: one key, a full block ± 1, L − 1, L, none


def _ragged(L):
    """[K,B] key counts: 1, inside, L, L − 1, one past a 32-key block, a few short of L."""
    return ((1, max(L // 2, 1), L), (max(L - 1, 1), min(33, L), max(L - 5, 1)))


@functools.lru_cache(maxsize=None)
def _case(kind, L, dh, dtype, kv, drop_p, heads=H, spike_block=0):
    """CPU inputs (rounded to `dtype`) and the float64 oracle of one case. kv: None, or [K,B] as a
    tuple of tuples. Shared between the tests (and the two implementations) that run the case."""
    seed = 1000 * L + dh
    if kind == "smooth":
        q, k, v, do = ac.smooth(K, B, heads, L, dh, seed=seed, dtype=dtype)
    else:
        q, k, v, do = ac.peaked(K, B, heads, L, dh, spike_block, seed=seed, dtype=dtype)
    kvt = None if kv is None else torch.tensor(kv, dtype=torch.int32)
    drop = ac.drop_factor(q.shape, SEEDS, drop_p)
    exact = (*ac.attn_fwd64(q, k, v, kvt, drop), *ac.attn_bwd64(do, q, k, v, kvt, drop))
    return (q, k, v, do), kvt, exact


def _dr(drop_p):
    return {"drop_p": drop_p, "drop_seeds": SEEDS.to(DEV)} if drop_p else {}


def _run(hip, inputs, kvt, drop_p=0.0):
    q, k, v, do = (t.to(DEV) for t in inputs)
    kv = None if kvt is None else kvt.to(DEV)
    o, lse = hip.attn_fwd(q, k, v, kv, **_dr(drop_p))
    dq, dk, dv = hip.attn_bwd(do, q, k, v, o, lse, kv, **_dr(drop_p))
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def _run_packed(hip, inputs, kvt, heads, drop_p=0.0):
    """The same case through the packed layout: qkv [K,B,L,3D] in, o [K,B,L,D] and dqkv out."""
    q, k, v, do = inputs
    D = heads * q.shape[-1]
    qkv = torch.cat([ac.flat(t) for t in (q, k, v)], -1).to(DEV)
    kv = None if kvt is None else kvt.to(DEV)
    o, lse = hip.attn_fwd_packed(qkv, heads, kv, **_dr(drop_p))
    dqkv = hip.attn_bwd_packed(ac.flat(do).to(DEV), qkv, o, lse, heads, kv, **_dr(drop_p))
    torch.cuda.synchronize()
    assert o.shape == (K, B, q.shape[-2], D) and dqkv.shape == qkv.shape
    return (ac.heads(o, heads), lse, *(ac.heads(g, heads) for g in dqkv.split(D, dim=-1)))


def _name(dtype):
    return "fp32" if dtype == torch.float32 else "bf16"


def _check(hip, group, valu, kind, L, dh, dtype, kv, drop_p=0.0, heads=H, spike_block=0, packed=False, **kw):
    inputs, kvt, exact = _case(kind, L, dh, dtype, kv, drop_p, heads, spike_block)
    tol, gtol = ac.tols(dtype, valu)
    what = (f"{group} {_name(dtype)} {'valu' if valu else 'mfma'}{' packed' if packed else ''} {kind} L={L} dh={dh} "
            f"kv={'none' if kv is None else 'set'} p={drop_p} blk={spike_block}")
    with ac.attn_mfma_option(hip, 0 if valu else 1):
        if valu:
            assert not hip.attn_packed_supported(L, dh)  # the packed layouts exist on the MFMA kernels only
        got = _run_packed(hip, inputs, kvt, heads, drop_p) if packed else _run(hip, inputs, kvt, drop_p)
    return ac.check_attention(got, exact, kvt, tol, gtol, what, **kw)


# ------------------------------------------------------------------------ VALU fallback
VALU_CASES = [(37, 8), (37, 16), (37, 20), (37, 32), (37, 64),
              (300, 64),  # 153 600 B (fwd, dq) and 156 000 B (dkv) of dynamic LDS, one 320-thread workgroup
              (300, 20),
              (513, 20)]  # two 320-row blocks per head, the second's last wave holding one row


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("L,dh", VALU_CASES)
def test_valu_fallback(hip, L, dh, dtype):
    _check(hip, "valu", True, "smooth", L, dh, dtype, _ragged(L))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_valu_fallback_without_key_mask(hip, dtype):
    _check(hip, "valu", True, "smooth", 37, 20, dtype, None)


def test_valu_fallback_refuses_dropout(hip):
    """The VALU kernels have no dropout: asking for it raises, it never returns an undropped result."""
    (q, k, v, do), kvt, _ = _case("smooth", 37, 20, torch.float32, _ragged(37), 0.0)
    q, k, v, do = (t.to(DEV) for t in (q, k, v, do))
    with ac.attn_mfma_option(hip, 0):
        o, lse = hip.attn_fwd(q, k, v, kvt.to(DEV))
        with pytest.raises(NotImplementedError):
            hip.attn_fwd(q, k, v, kvt.to(DEV), **_dr(0.1))
        with pytest.raises(NotImplementedError):
            hip.attn_bwd(do, q, k, v, o, lse, kvt.to(DEV), **_dr(0.1))


# ------------------------------------------------------------------------ dh = 48 (MFMA, DPAD 64)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("L", [37, 130])
@pytest.mark.parametrize("packed", [False, True], ids=["unpacked", "packed"])
def test_head_dim_48(hip, packed, L, drop_p, dtype):
    """dh = 48 (D = 192, 4 heads): columns 48-63 of the padded tile are zeros on the way in and are
    not stored on the way out — a leak would land in the next head's columns (packed rows) or in the
    next row (contiguous heads), which are compared with the oracle like every other element."""
    assert hip.attn_packed_supported(L, 48)
    _check(hip, "dh48", False, "smooth", L, 48, dtype, _ragged(L), drop_p, heads=4, packed=packed)


# ------------------------------------------------------------------------ block edges
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("valu", [False, True], ids=["mfma", "valu"])
def test_key_count_edges(hip, valu, dh, dtype):
    """L = 129 (a trailing workgroup with one row) with 1, 32, 33, 128, 129 and 0 valid keys: a dK/dV
    workgroup whose keys are all padding, and a sequence without a key (exact zeros, nothing NaN)."""
    errs = _check(hip, "edges", valu, "smooth", 129, dh, dtype, KV_EDGE)
    assert set(errs) == {"o", "lse", "dq", "dk", "dv"}


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("full_kv", [False, True], ids=["kv_none", "kv_L"])
@pytest.mark.parametrize("L", [1, 32, 33])
@pytest.mark.parametrize("valu", [False, True], ids=["mfma", "valu"])
def test_sequence_length_edges(hip, valu, L, full_kv, dtype):
    """One key, exactly one 32-key block, one key past it; without a mask and with kv = L. At L = 1 dq
    and dk are exactly 0 as the difference of dP = dO·v and δ = dO·o (o = v), which the kernels form by
    different routes (an MFMA product and an fp32 dot): there the gradient bound is taken relative to
    the terms that cancel, max Σ|dO||v| · max |k| (or |q|) / √dh, instead of to max |exact| = 0."""
    dh = 32
    kv = ((L,) * B,) * K if full_kv else None
    kw = {}
    if L == 1:
        (q, k, v, do), _, _ = _case("smooth", L, dh, dtype, kv, 0.0)
        terms = (ac.d(do).abs() * ac.d(v).abs()).sum(-1).max().item() / dh ** 0.5
        kw["cancel_scale"] = {"dq": terms * ac.d(k).abs().max().item(), "dk": terms * ac.d(q).abs().max().item()}
    _check(hip, "edges", valu, "smooth", L, dh, dtype, kv, **kw)


# ------------------------------------------------------------------------ peaked softmax
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("spike_block", [0, 4], ids=["first_block", "last_block"])
@pytest.mark.parametrize("dh", [16, 64])
def test_peaked_softmax_mfma(hip, dh, spike_block, drop_p, dtype):
    """Scores in the tens (attention_common.peaked). The row maximum in the first key block: the later
    blocks' probabilities underflow (the `p != 0` shortcut in front of the dropout hash takes its other
    side) and corr = 1. In the last block, which holds one key at L = 129: everything accumulated before
    it is rescaled by corr = exp(m − mn), many powers of e below 1."""
    _check(hip, "peaked", False, "peaked", 129, dh, dtype, None, drop_p, spike_block=spike_block)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("spike_block", [0, 4], ids=["first_block", "last_block"])
def test_peaked_softmax_valu(hip, spike_block, dtype):
    _check(hip, "peaked", True, "peaked", 129, 16, dtype, None, spike_block=spike_block)


# ------------------------------------------------------------------------ unpacked dropout
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("L,dh", [(37, 20), (130, 64)])
def test_unpacked_dropout(hip, L, dh, dtype):
    """`hip.attn_fwd` / `attn_bwd` with dropout on [K,B,H,L,dh], per-client seeds, B·H = 6 heads per
    client (the hash takes head % hpc and seeds[head / hpc]): forward and backward against the oracle."""
    _check(hip, "dropout", False, "smooth", L, dh, dtype, _ragged(L), 0.1)


# ------------------------------------------------------------------------ predicates
@pytest.mark.parametrize("opt", [0, 1], ids=["attn_mfma_0", "attn_mfma_1"])
def test_attn_supported_is_what_the_launcher_does(hip, opt):
    """`attn_supported(L, dh)` is true exactly when `hip.attn_fwd` runs, under both option values:
    dh 48 has no VALU kernel, (700, 64) needs 358 KB of LDS there, (300, 64) just fits."""
    expect = {(37, 48): bool(opt), (700, 64): bool(opt), (700, 8): True, (300, 64): True, (37, 20): True}
    with ac.attn_mfma_option(hip, opt):
        for (L, dh), want in expect.items():
            q = torch.randn(1, 1, 1, L, dh, device=DEV)
            supported = bool(hip._C.attn_supported(L, dh))
            try:
                o, lse = hip.attn_fwd(q, q, q)
                torch.cuda.synchronize()
                ran = bool(torch.isfinite(o).all() and torch.isfinite(lse).all())
            except NotImplementedError:
                ran = False
            assert supported == ran == want, (opt, L, dh, supported, ran)
            assert hip.attn_packed_supported(L, dh) == (bool(opt) and dh in (8, 16, 20, 32, 48, 64))
