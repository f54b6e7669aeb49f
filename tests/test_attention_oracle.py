"""The fp32 CPU attention of `ops.ref` (the CPU backend of the Transformer, and what the older GPU
tests compare the kernels with) against the float64 oracle of tests/attention_common.py, and the
kv = 0 contract: a sequence without a valid key gives o = 0, lse = 0 and zero gradients, and leaves the
rest of the batch untouched. Runs without a GPU."""

import pytest
import torch

import attention_common as ac
from distributed_learning_simulator_amd.ops import functional as Fn
from distributed_learning_simulator_amd.ops import ref

K, B, H = 2, 3, 2
SEEDS = torch.tensor([5, -9], dtype=torch.int32)


def _kv(L):
    """key_valid [K,B] holding 1, 32, 33 and L wherever they fit into L."""
    vals = [1, min(32, L), min(33, L), L, max(L - 1, 1), L]
    return torch.tensor(vals, dtype=torch.int32).reshape(K, B)


def _run_ref(q, k, v, do, kv, drop_p):
    dr = {"drop_p": drop_p, "drop_seeds": SEEDS} if drop_p else {}
    o, lse = ref.attn_fwd(q, k, v, kv, **dr)
    return (o, lse, *ref.attn_bwd(do, q, k, v, o, lse, kv, **dr))


def _oracle(q, k, v, do, kv, drop_p):
    drop = ac.drop_factor(q.shape, SEEDS, drop_p)
    return (*ac.attn_fwd64(q, k, v, kv, drop), *ac.attn_bwd64(do, q, k, v, kv, drop))


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("L,dh", [(37, 20), (129, 32), (33, 64)])
def test_ref_smooth(L, dh, masked, drop_p):
    q, k, v, do = ac.smooth(K, B, H, L, dh, seed=L + dh)
    kv = _kv(L) if masked else None
    ac.check_attention(_run_ref(q, k, v, do, kv, drop_p), _oracle(q, k, v, do, kv, drop_p), kv, ac.REF_TOL,
                       ac.REF_TOL, f"ref smooth L={L} dh={dh} kv={masked} p={drop_p}")


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("spike_block", [0, 4])
@pytest.mark.parametrize("dh", [16, 64])
def test_ref_peaked(dh, spike_block, masked, drop_p):
    """Scores in the tens, the row maximum in the first or in the last (one-key) block. With a key mask
    the spike of the last block is masked for every sequence but the full ones: both cases count."""
    L = 129
    q, k, v, do = ac.peaked(K, B, H, L, dh, spike_block, seed=dh + spike_block)
    kv = _kv(L) if masked else None
    ac.check_attention(_run_ref(q, k, v, do, kv, drop_p), _oracle(q, k, v, do, kv, drop_p), kv, ac.REF_TOL,
                       ac.REF_TOL, f"ref peaked dh={dh} block={spike_block} kv={masked} p={drop_p}")


def test_oracle_against_float64_autograd():
    """The oracle's backward is the derivative of its forward (float64 autograd through the plainly
    written forward), dropout factor and key mask included."""
    L, dh = 37, 20
    q, k, v, do = (t.double().requires_grad_() for t in ac.smooth(K, B, H, L, dh, seed=3))
    kv = _kv(L)
    drop = ac.drop_factor(q.shape, SEEDS, 0.1).double()
    s = torch.matmul(q, k.transpose(-1, -2)) / dh ** 0.5
    s = s.masked_fill(torch.arange(L)[None, None, None, None, :] >= kv.long()[:, :, None, None, None], float("-inf"))
    o = torch.matmul(torch.softmax(s, -1) * drop, v)
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), do.detach())
    o64, lse64 = ac.attn_fwd64(q, k, v, kv, drop)
    assert ac.rel_err(o64, o) < 1e-13
    assert ac.rel_err(lse64, torch.logsumexp(s, -1)) < 1e-13
    for a, b in zip(ac.attn_bwd64(do, q, k, v, kv, drop), (gq, gk, gv)):
        assert ac.rel_err(a, b) < 1e-12


# ------------------------------------------------------------------------ kv = 0
KV_EDGE = torch.tensor([[1, 32, 33], [128, 129, 0]], dtype=torch.int32)


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_ref_empty_sequence_contract(drop_p):
    """One sequence without a valid key: exact zeros for it (o, lse, dq, dk, dv), nothing non-finite in
    the batch, and the other sequences against the oracle (fails with NaN before the ops/ref.py fix)."""
    L, dh = 129, 32
    q, k, v, do = ac.smooth(K, B, H, L, dh, seed=11)
    got = _run_ref(q, k, v, do, KV_EDGE, drop_p)
    for t in got:
        assert torch.isfinite(t).all()
    ac.check_attention(got, _oracle(q, k, v, do, KV_EDGE, drop_p), KV_EDGE, ac.REF_TOL, ac.REF_TOL,
                       f"ref kv=0 p={drop_p}")


@pytest.mark.parametrize("axis", ["batch", "client"])
def test_ref_empty_sequence_leaves_the_others_bitwise(axis):
    """The sequences beside an empty one have the bits they have when it is not in the batch."""
    L, dh = 37, 20
    if axis == "batch":
        q, k, v, do = ac.smooth(1, 3, H, L, dh, seed=12)
        kv = torch.tensor([[5, 0, L]], dtype=torch.int32)
        keep = lambda t: t[:, [0, 2]]  # noqa: E731
    else:
        q, k, v, do = ac.smooth(2, 1, H, L, dh, seed=13)
        kv = torch.tensor([[L - 4], [0]], dtype=torch.int32)
        keep = lambda t: t[:1]  # noqa: E731
    full = _run_ref(q, k, v, do, kv, 0.0)
    part = _run_ref(*(keep(t).contiguous() for t in (q, k, v, do)), keep(kv).contiguous(), 0.0)
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), full, part):
        assert torch.equal(keep(a), b), name
    gone = kv <= 0
    for a in full:
        assert torch.all(a[gone] == 0)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_functional_attention_with_an_empty_sequence(packed, drop_p):
    """`functional.attention` / `attention_packed` on the CPU under autograd: one empty sequence leaves
    every other sequence's output and gradients finite and equal to the oracle's, its own exactly 0."""
    L, dh = 37, 16
    kv = torch.tensor([[1, 32, 33], [L, L - 1, 0]], dtype=torch.int32)
    q, k, v, do = ac.smooth(K, B, H, L, dh, seed=21)
    dr = {"drop_p": drop_p, "drop_seeds": SEEDS} if drop_p else {}
    if packed:
        qkv = torch.cat([ac.flat(t) for t in (q, k, v)], -1).requires_grad_()
        o = Fn.attention_packed(qkv, kv, H, **dr)
        o.backward(ac.flat(do))
        D = H * dh
        o = ac.heads(o, H)
        grads = [ac.heads(g, H) for g in qkv.grad.split(D, dim=-1)]
    else:
        q, k, v = (t.requires_grad_() for t in (q, k, v))
        o = Fn.attention(q, k, v, kv, **dr)
        o.backward(do)
        grads = [q.grad, k.grad, v.grad]
    q, k, v = (t.detach() for t in (q, k, v))
    drop = ac.drop_factor(q.shape, SEEDS, drop_p)
    o64, lse64 = ac.attn_fwd64(q, k, v, kv, drop)
    # (lse is not an output of the functional layer: the oracle's stands in, so the comparison covers o
    # and the three gradients)
    ac.check_attention((o, lse64, *grads), (o64, lse64, *ac.attn_bwd64(do, q, k, v, kv, drop)), kv, ac.REF_TOL,
                       ac.REF_TOL, f"functional packed={packed} p={drop_p}")
