"""The secure-aggregation kernels (csrc/secagg.hip) against the CPU oracle (ops/ref.py) on the MI355X: masked rows
and counters, the ring sum and the unmasking bit for bit, operands as views inside guarded buffers, in place
and out of place, and a session against the oracle on its own uploads."""

import functools
import os
import sys

import pytest
import torch

from distributed_learning_simulator_amd.ops import fl, ref
from distributed_learning_simulator_amd.utils import secagg_protocol as SP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_secagg_sessions as TS  # noqa: E402  (the session spies and the round oracle)

pytestmark = pytest.mark.gpu

R, F = 1.0, 20
GUARD = 64
NAN, INF = float("nan"), float("inf")
KINDS = ("gauss", "beyond", "ties", "tiny", "nonfinite")
ENTRY_COUNTS = (0, 1, 2, 99, 511)


def _key(i):
    return (0x9E3779B97F4A7C15 * (i + 1) + (i << 40)) & (2 ** 64 - 1)


def _data(kind, K, P, seed=0):
    g = torch.Generator().manual_seed(1000 * K + P + seed)
    if kind == "gauss":
        return torch.randn((K, P), generator=g) * 0.4  # a few per cent beyond ±R
    if kind == "beyond":
        return (torch.randn((K, P), generator=g).sign() + 0.0) * (1.5 + torch.rand((K, P), generator=g))
    if kind == "ties":  # odd multiples of half a unit: every element is a tie
        return (torch.randint(-2 ** 19, 2 ** 19, (K, P), generator=g) * 2 + 1).float() * 2.0 ** -(F + 1)
    if kind == "tiny":
        pool = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 2.0 ** -(F + 1), 2.0 ** -(F + 2)])
        return pool[torch.randint(0, len(pool), (K, P), generator=g)]
    pool = torch.tensor([NAN, INF, -INF, 0.25, -NAN, 3e38])
    return pool[torch.randint(0, len(pool), (K, P), generator=g)]


def _entries(K, counts):
    """A ragged table: row k owns counts[k % len(counts)] entries with distinct keys and mixed signs."""
    offsets, keys, signs = [0], [], []
    for k in range(K):
        n = counts[k % len(counts)]
        keys += [_key(1000 * k + e) for e in range(n)]
        signs += [1 if (e * 7 + k) % 3 else -1 for e in range(n)]
        offsets.append(len(keys))
    return offsets, keys, signs


@functools.lru_cache(maxsize=None)
def _oracle(kind, K, P, counts):
    """(x, entries, words, counters) on the CPU, computed once per case and never modified."""
    x = _data(kind, K, P)
    entries = _entries(K, counts)
    words, counters = ref.secagg_mask_rows(x, *entries, R, F)
    return x, entries, words, counters


def _span():
    from distributed_learning_simulator_amd.ops import hip

    return hip.secagg_mask_span()


def _launch(x, entries, P, strided, in_place):
    """x inside a guarded device buffer (row stride P + 16 if strided), the upload in place or into a guarded
    int32 buffer. Returns (words, counters, ok) — ok: guards and read-only inputs held."""
    K = x.shape[0]
    ld = P + 16 if strided else P
    wide = torch.full((GUARD + K * ld + GUARD,), 7.0, device="cuda")
    xv = wide[GUARD : GUARD + K * ld].view(K, ld)[:, :P]
    xv.copy_(x.cuda())
    before = wide.clone()
    if in_place:
        words, counters = fl.secagg_mask_rows(xv, entries, R, F, out=xv.view(torch.int32))
        assert words.data_ptr() == xv.data_ptr()
        seven = torch.tensor(7.0).view(torch.int32).item()
        iw = wide.view(torch.int32)
        ok = bool((iw[:GUARD] == seven).all() and (iw[GUARD + K * ld :] == seven).all())
        if strided:  # the columns past P of every row
            ok = ok and bool((iw[GUARD : GUARD + K * ld].view(K, ld)[:, P:] == seven).all())
        return words, counters, ok
    owide = torch.full((GUARD + K * ld + GUARD,), -5, dtype=torch.int32, device="cuda")
    ov = owide[GUARD : GUARD + K * ld].view(K, ld)[:, :P]
    words, counters = fl.secagg_mask_rows(xv, entries, R, F, out=ov)
    assert words is ov
    ok = bool((owide[:GUARD] == -5).all() and (owide[GUARD + K * ld :] == -5).all())
    if strided:
        ok = ok and bool((owide[GUARD : GUARD + K * ld].view(K, ld)[:, P:] == -5).all())
    ok = ok and torch.equal(wide.view(torch.int32), before.view(torch.int32))  # x is read-only
    return words, counters, ok


# ------------------------------------------------------------------ secagg_mask_rows
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("P", [16, 48, 4112])
@pytest.mark.parametrize("K", [1, 3, 13])
def test_mask_rows_equal_the_oracle(hip, K, P, in_place, strided):
    """Ragged entry tables over {0, 1, 2, 99, 511} (rotated with K so that a lone row gets 511 at P = 16 and 99
    otherwise); the data kind rotates with the case, and every kind meets every P below."""
    counts = ENTRY_COUNTS[::-1] if (K == 1 and P == 16) else ENTRY_COUNTS[3:] + ENTRY_COUNTS[:3] if K == 1 else ENTRY_COUNTS
    kind = KINDS[(K + P // 16 + 2 * in_place + strided) % len(KINDS)]
    x, entries, want, counters = _oracle(kind, K, P, counts)
    words, got_counters, ok = _launch(x, entries, P, strided, in_place)
    assert ok
    assert torch.equal(words.cpu(), want) and torch.equal(got_counters.cpu(), counters)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [16, 48, 4112])
def test_mask_rows_data_kinds(hip, kind, P):
    x, entries, want, counters = _oracle(kind, 3, P, (2, 0, 99))
    for variant in (None, 1, 2, 3):  # every ILP form of the expander gives the same bits
        words, got = fl.secagg_mask_rows(x.cuda(), entries, R, F, variant=variant)
        assert torch.equal(words.cpu(), want) and torch.equal(got.cpu(), counters)
    if kind == "beyond":
        assert counters[:, 0].tolist() == [P] * 3
    if kind == "nonfinite":
        assert (counters[:, 1] > 0).all() and (counters[:, 0] > 0).all()
    if kind in ("ties", "tiny"):
        assert not counters.any()


def test_mask_rows_second_trip_of_the_grid_stride_loop(hip):
    """P = one full grid's span + 16: the block cap of the mask kernel is 1024 workgroups of 256 lanes a row, each lane
    owning groups of four elements, so the last 16 elements are the first lanes' second trip."""
    P = _span() + 16
    assert P % 16 == 0 and P > 1024 * 256 * 4
    for K, counts in ((1, (2,)), (3, (1, 0, 2))):
        x, entries, want, counters = _oracle("gauss", K, P, counts)
        a, ca, ok = _launch(x, entries, P, strided=False, in_place=True)
        assert ok and torch.equal(a.cpu(), want) and torch.equal(ca.cpu(), counters)
        b, cb = fl.secagg_mask_rows(x.cuda(), entries, R, F)  # two launches, bitwise equal
        assert torch.equal(a, b) and torch.equal(ca, cb)
    for variant in (1, 2, 3):
        P = hip.secagg_mask_span(variant) + 16
        x, entries, want, counters = _oracle("gauss", 1, P, (1,))
        words, got = fl.secagg_mask_rows(x.cuda(), entries, R, F, variant=variant)
        assert torch.equal(words.cpu(), want) and torch.equal(got.cpu(), counters)


def test_refusals_on_the_device(hip):
    x = torch.zeros(4, 16, device="cuda")
    none = ([0, 0, 0, 0, 0], [], [])
    for out in (torch.zeros(4, 16, device="cuda"), torch.zeros(4, 12, dtype=torch.int32, device="cuda"),
                torch.zeros(68, dtype=torch.int32, device="cuda")[1:65].view(4, 16), torch.zeros(4, 16, dtype=torch.int32)):
        with pytest.raises(ValueError):
            fl.secagg_mask_rows(x, none, 1.0, 8, out=out)
    with pytest.raises(ValueError):
        fl.secagg_mask_rows(torch.zeros(513, 4, device="cuda"), ([0] * 514, [], []), 1.0, 8)
    with pytest.raises(ValueError):
        fl.ring_sum(torch.zeros(513, 16, dtype=torch.int32, device="cuda"), torch.zeros(16, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------ ring_sum / ring_unmask
@pytest.mark.parametrize("n", [1, 13, 100, 512])
def test_ring_sum_into_a_nonzero_accumulator(hip, n):
    P = 4112
    g = torch.Generator().manual_seed(n)
    rows = torch.randint(-2 ** 31, 2 ** 31, (n, P + 16), generator=g, dtype=torch.int64).to(torch.int32)
    rows[:, 0] = 2 ** 31 - 1
    rows[:, 1] = -2 ** 31
    rows[n // 2, 2] = -2 ** 31
    rows[0, 3] = 2 ** 31 - 1
    acc0 = torch.randint(-2 ** 40, 2 ** 40, (P,), generator=g, dtype=torch.int64)
    want = ref.ring_sum(rows[:, :P], acc0.clone())
    assert want[0] == acc0[0] + n * (2 ** 31 - 1) and want[1] == acc0[1] - n * 2 ** 31
    wide = torch.full((GUARD + P + GUARD,), 7, dtype=torch.int64, device="cuda")
    acc = wide[GUARD : GUARD + P]
    acc.copy_(acc0)
    drows = rows.cuda()
    before = drows.clone()
    assert fl.ring_sum(drows[:, :P], acc) is acc  # strided rows
    assert torch.equal(acc.cpu(), want) and torch.equal(drows, before)
    assert (wide[:GUARD] == 7).all() and (wide[GUARD + P :] == 7).all()
    again = acc0.cuda()
    fl.ring_sum(drows[:, :P].contiguous(), again)
    assert torch.equal(again, acc)


@pytest.mark.parametrize("E", [1, 700])
def test_ring_unmask(hip, E):
    P = 4112
    keys = [_key(e) for e in range(E)]
    signs = [1 if e % 3 else -1 for e in range(E)]
    acc0 = torch.randint(-2 ** 40, 2 ** 40, (P,), generator=torch.Generator().manual_seed(E), dtype=torch.int64)
    want = ref.ring_unmask(acc0.clone(), keys, signs)
    wide = torch.full((GUARD + P + GUARD,), 7, dtype=torch.int64, device="cuda")
    for variant in (None, 1, 3):
        acc = wide[GUARD : GUARD + P]
        acc.copy_(acc0)
        assert fl.ring_unmask(acc, (keys, signs), variant=variant) is acc
        assert torch.equal(acc.cpu(), want)
        assert (wide[:GUARD] == 7).all() and (wide[GUARD + P :] == 7).all()
    assert torch.equal(fl.ring_unmask(acc0.cuda(), ([], [])).cpu(), acc0)


def test_cancellation_and_recovery_on_the_device(hip):
    n, P = 13, 4112
    ids = list(range(n))
    proto = SP.RoundProtocol(seed=3, rnd=5, selected=ids, degree=4, threshold=2)
    Rn, f = fl.secagg_frac_bits(1.0, n)
    x = _data("gauss", n, P, seed=9)
    x[:, 4100:] = 0
    q, _ = ref.secagg_quantise(x, Rn, f)
    buf = x.cuda()
    words, _ = fl.secagg_mask_rows(buf, proto.entry_table(ids), Rn, f, out=buf.view(torch.int32))
    for dropped in ([], [6], [6, 7]):
        S = [c for c in ids if c not in dropped]
        keys, signs, aborted = proto.recover(S)
        assert not aborted
        acc = torch.zeros(P, dtype=torch.int64, device="cuda")
        fl.ring_sum(words[: len(S) // 2] if not dropped else words[S[: len(S) // 2]].contiguous(), acc)
        fl.ring_sum(words[len(S) // 2 :] if not dropped else words[S[len(S) // 2 :]].contiguous(), acc)
        fl.ring_unmask(acc, (keys, signs))
        dec = fl.ring_decode(acc, f)
        assert dec.is_cuda and torch.equal(dec.cpu(), q[S].sum(0).double() * 2.0 ** -f)
        assert (dec[4100:] == 0).all()


# ------------------------------------------------------------------ session
def test_gpu_session_equals_oracle_on_its_uploads(hip, tmp_path, monkeypatch):
    """Two rounds of 8 clients with failure_rate 0.3: seed 0 drops client 6 in round 1 and client 2 in round 2 (the
    injection does not depend on the device). Every uploaded row and θ_{t+1} bit for bit."""
    rounds, uploads = [], []
    TS._spy(monkeypatch, rounds, uploads)
    ov = {"round": 2, "worker_number": 8, "dataset_kwargs.scale": 0.02, "save_models": False,
          "algorithm_kwargs.failure_rate": 0.3, "algorithm_kwargs.secagg_range": 0.05}
    sess, _ = TS._run(ov, tmp_path, "cuda")
    Rn, f = fl.secagg_frac_bits(0.05, 8)
    assert len(rounds) == 2 and sess.server.global_parameter.is_cuda and [r["dropped"] for r in rounds] == [[6], [2]]
    valid = sess.layout.valid_mask()
    for r, waves in zip(rounds, TS._by_round(uploads, rounds)):
        exp = TS._oracle_round(r, waves, sess.config.seed, Rn, f)
        assert torch.equal(TS._bits64(r["new64"]), TS._bits64(exp)) and torch.equal(r["new"], exp.float())
        assert r["stats"]["secagg_aborted"] == 0
    assert torch.isfinite(sess.server.global_parameter).all()
    assert (sess.server.global_parameter.cpu()[~valid].view(torch.int32) == 0).all()  # padding stays +0
