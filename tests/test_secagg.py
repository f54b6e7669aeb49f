"""Secure aggregation primitives on the CPU: the mask stream, the fixed-point code, cancellation in Z_{2^32},
dropout recovery and the refusals (ops/fl.py secagg_mask_rows / ring_sum / ring_unmask / ring_decode, oracle
ops/ref.py; the protocol layer has its own file)."""

import math
import struct

import pytest
import torch

from distributed_learning_simulator_amd.ops import fl, ref
from distributed_learning_simulator_amd.utils import secagg_protocol as SP

M32 = 0xFFFFFFFF
KEY = 0x9E3779B97F4A7C15  # both halves non-zero


def _w(key, p):
    """w(κ, p) restated with the public Philox oracle, one position at a time."""
    i = p // 4
    words = ref.philox4x32((i & M32, i >> 32, 0, 0x53413031), (key & M32, key >> 32))
    return int(words[p % 4])


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _rows(n, P, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, P), generator=g) * scale


# ------------------------------------------------------------------ mask stream
@pytest.mark.parametrize("key", [KEY, 1, 0xFFFFFFFF00000000, 0])
def test_mask_word_is_the_philox_word_of_its_position(key):
    P = 64
    got = fl.secagg_mask_words(key, P).tolist()
    for p in (0, 1, 2, 3, 4, 5, 6, 7, 17, 42, 63):  # every p % 4
        assert got[p] == _w(key, p) and 0 <= got[p] <= M32
    assert len(set(got)) > 60  # (not a constant stream)


def test_mask_words_depend_on_key_and_position_alone():
    whole = fl.secagg_mask_words(KEY, 4099)
    for start, n in ((0, 5), (1, 4), (2, 9), (3, 1), (4094, 5), (1001, 2047)):
        assert torch.equal(fl.secagg_mask_words(KEY, n, start=start), whole[start : start + n])
    p = 2 ** 34 + 6  # the second counter word is in use
    assert int(fl.secagg_mask_words(KEY, 1, start=p)[0]) == _w(KEY, p)
    assert not torch.equal(fl.secagg_mask_words(KEY + 1, 64), whole[:64])


# ------------------------------------------------------------------ fixed point
def _q_python(x, R, f):
    """q(x) with python floats: the clamp in fp32 (R is an fp32 value), one rounding to nearest even."""
    if math.isnan(x):
        return 0
    t = max(-R, min(R, x))
    return round(t * 2.0 ** f)  # python's round is half-to-even; t · 2^f is exact


def test_frac_bits_is_the_largest_that_cannot_wrap():
    assert fl.secagg_frac_bits(1.0, 1) == (1.0, 30)
    assert fl.secagg_frac_bits(1.0, 512) == (1.0, 21)  # 512 · 2^21 = 2^30; 2^22 would give 2^31 > 2^31 − 1
    assert fl.secagg_frac_bits(0.5, 1) == (0.5, 31)
    assert fl.secagg_frac_bits(3.0, 10)[1] == 26  # 30 · 2^26 = 2.01e9 ≤ 2^31 − 1 < 30 · 2^27
    R, f = fl.secagg_frac_bits(0.1, 7)
    assert R == _f32(0.1) and 7 * R * 2.0 ** f <= 2 ** 31 - 1 < 7 * R * 2.0 ** (f + 1)
    assert fl.secagg_frac_bits(1.0, 512, 21) == (1.0, 21) and fl.secagg_frac_bits(1.0, 512, 3) == (1.0, 3)


@pytest.mark.parametrize("m", [1, 512])
def test_quantisation_against_python_rounding(m):
    R, f = fl.secagg_frac_bits(1.0, m)
    u = 2.0 ** -f
    vals = [0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u, 3.5 * u, 0.49 * u, 0.51 * u,  # ties and near
            R, -R, _f32(1.0000001), _f32(-1.0000001), 7.0, -7.0, math.inf, -math.inf, math.nan,
            0.0, -0.0, 1e-45, -1e-45, 1e-39, 0.3, -0.7, 0.99999994]
    assert len(vals) % 4 == 2
    vals += [0.0, 0.0]
    x = torch.tensor([vals, vals[::-1]], dtype=torch.float32)
    out, stats = fl.secagg_mask_rows(x, ([0, 0, 0], [], []), R, f)
    assert out.dtype == torch.int32 and stats.dtype == torch.int32
    for row, src in zip(out.tolist(), x.tolist()):
        assert row == [_q_python(v, R, f) for v in src]
    assert out[0, 0] == 0 and out[0, 1] == 2 and out[0, 2] == 2 and out[0, 4] == -2 and out[0, 6] == 4  # ties to even
    top = round(R * 2.0 ** f)
    assert out[0, 9] == top and out[0, 10] == -top and out[0, 15] == top and out[0, 16] == -top
    assert m * top <= 2 ** 31 - 1
    assert stats.tolist() == [[6, 1], [6, 1]]  # just outside ±R (2), ±7 (2), ±inf (2); one NaN


# ------------------------------------------------------------------ cancellation
def _masked(x, proto, clients, R, f):
    return fl.secagg_mask_rows(x, proto.entry_table(clients), R, f)[0]


def _self_masks(proto, clients):
    keys = [proto.secrets[c][1] for c in clients if proto.partners[c]]
    return keys, [1] * len(keys)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 13])
@pytest.mark.parametrize("d", [0, 2, 4])
def test_pair_masks_cancel_in_the_ring_sum(n, d):
    P, valid = 48, 41  # the last 7 positions are layout padding: x = 0 there
    ids = list(range(3, 3 + n))
    proto = SP.RoundProtocol(seed=11, rnd=2, selected=ids, degree=d)
    R, f = fl.secagg_frac_bits(1.0, n)
    x = _rows(n, P, 100 * n + d)
    x[:, valid:] = 0
    x[0, 5] = 9.0  # clamped
    rows = _masked(x, proto, ids, R, f)
    q, _ = ref.secagg_quantise(x, R, f)
    if n > 1:
        assert (rows.long() != q).any(1).all()  # every row is masked ...
    acc = fl.ring_sum(rows, torch.zeros(P, dtype=torch.int64))
    fl.ring_unmask(acc, _self_masks(proto, ids))
    dec = fl.ring_decode(acc, f)
    assert torch.equal(dec, q.sum(0).double() * 2.0 ** -f)  # ... and the sum is exact
    assert (dec[valid:] == 0).all() and (dec[valid:].view(torch.int64) == 0).all()
    # order freedom: permuted rows, and two ring_sum calls
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    acc2 = fl.ring_sum(rows[perm].contiguous(), torch.zeros(P, dtype=torch.int64))
    acc3 = torch.zeros(P, dtype=torch.int64)
    if n > 1:
        fl.ring_sum(rows[n // 2 :], acc3)
        fl.ring_sum(rows[: n // 2], acc3)
    else:
        fl.ring_sum(rows, acc3)
    for other in (acc2, acc3):
        fl.ring_unmask(other, _self_masks(proto, ids))
        assert torch.equal(other, acc)


def _recovery_case(n, d, dropped, threshold=None):
    P = 32
    ids = list(range(n))
    proto = SP.RoundProtocol(seed=5, rnd=1, selected=ids, degree=d, threshold=threshold)
    R, f = fl.secagg_frac_bits(1.0, n)
    x = _rows(n, P, 7 * n + d)
    rows = _masked(x, proto, ids, R, f)
    q, _ = ref.secagg_quantise(x, R, f)
    S = [c for c in ids if c not in dropped]
    keys, signs, aborted = proto.recover(S)
    assert not aborted
    acc = fl.ring_sum(rows[S].contiguous(), torch.zeros(P, dtype=torch.int64))
    bare = acc.clone()
    fl.ring_unmask(acc, (keys, signs))
    assert torch.equal(fl.ring_decode(acc, f), q[S].sum(0).double() * 2.0 ** -f)
    # without the recovery entries (self masks only) the dropped clients' pair masks stay in the sum
    fl.ring_unmask(bare, _self_masks(proto, S))
    assert not torch.equal(fl.ring_decode(bare, f), fl.ring_decode(acc, f))
    assert len(keys) == len(S) + sum(len([j for j in proto.partners[x] if j in S]) for x in dropped)


@pytest.mark.parametrize("d", [0, 4])
def test_every_single_dropout_is_recovered(d):
    for c in range(8):
        _recovery_case(8, d, [c])


def test_two_adjacent_dropouts_on_the_degree_4_ring():
    # client 1 keeps two of its four partners (7 and 0): the default threshold 4 // 2 + 1 = 3 would abort
    # the round (test_secagg_protocol.py); with t = 2 the pair is recovered
    _recovery_case(8, 4, [2, 3], threshold=2)
    _recovery_case(8, 4, [7, 0], threshold=2)  # adjacent across the wrap
    assert SP.RoundProtocol(seed=5, rnd=1, selected=range(8), degree=4).recover([0, 1, 4, 5, 6, 7])[2]


# ------------------------------------------------------------------ a masked row looks uniform
def test_masked_row_bytes_look_uniform():
    P = 2 ** 20
    x = (torch.arange(P, dtype=torch.float32) % 17 - 8) * 2.0 ** -10  # small q
    R, f = fl.secagg_frac_bits(1.0, 1, 20)
    row, _ = fl.secagg_mask_rows(x[None], ([0, 1], [KEY], [1]), R, f)
    v = row[0].long() & M32
    for name, b in (("top", v >> 24), ("low", v & 0xFF)):
        counts = torch.bincount(b, minlength=256).double()
        chi2 = float(((counts - P / 256) ** 2 / (P / 256)).sum())
        print(f"chi2 of the {name} byte: {chi2:.1f}")
        assert chi2 < 255 + 5 * math.sqrt(510)
    q, _ = ref.secagg_quantise(x[None], R, f)
    low = torch.bincount(q[0] & 0xFF, minlength=256).double()  # (the clear code is anything but uniform)
    assert float(((low - P / 256) ** 2 / (P / 256)).sum()) > 1e5


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("R", [None, 0.0, -1.0, math.inf, math.nan, "x"])
def test_bad_range_is_refused(R):
    with pytest.raises((ValueError, TypeError)):
        fl.secagg_frac_bits(R, 4)


def test_frac_bits_that_overflow_the_ring_are_refused():
    with pytest.raises(ValueError, match="overflows the ring"):
        fl.secagg_frac_bits(1.0, 512, 22)
    with pytest.raises(ValueError, match="overflows the ring"):
        fl.secagg_frac_bits(1.0, 1, 31)
    with pytest.raises(ValueError):
        fl.secagg_frac_bits(1.0, 4, 0)
    with pytest.raises(ValueError, match="no fixed-point code"):
        fl.secagg_frac_bits(3e9, 1)
    with pytest.raises(ValueError):  # the op checks its own bound R · 2^f ≤ 2^31 − 1
        fl.secagg_mask_rows(torch.zeros(1, 4), ([0, 0], [], []), 4.0, 30)


def test_bad_graph_and_threshold_are_refused():
    with pytest.raises(ValueError, match="even"):
        SP.mask_graph(range(8), 3)
    with pytest.raises(ValueError):
        SP.mask_graph(range(8), -2)
    for t in (0, 5):
        with pytest.raises(ValueError, match="secagg_threshold"):
            SP.RoundProtocol(1, 1, range(8), degree=4, threshold=t)
    SP.RoundProtocol(1, 1, range(8), degree=4, threshold=4)


def test_bad_operands_are_refused():
    x = torch.zeros(4, 16)
    none = ([0, 0, 0, 0, 0], [], [])
    bad_outs = [torch.zeros(4, 16), torch.zeros(4, 12, dtype=torch.int32), torch.zeros(3, 16, dtype=torch.int32),
                torch.zeros(4 * 16 + 4, dtype=torch.int32)[1:65].view(4, 16),  # 4 B off a 16-B boundary
                torch.zeros(4, 18, dtype=torch.int32)[:, :16]]  # row stride 18: rows not 16-B aligned
    for out in bad_outs:
        with pytest.raises(ValueError):
            fl.secagg_mask_rows(x, none, 1.0, 8, out=out)
    with pytest.raises(ValueError):
        fl.secagg_mask_rows(torch.zeros(4, 18)[:, :16], none, 1.0, 8)
    with pytest.raises(ValueError):
        fl.secagg_mask_rows(torch.zeros(4, 16, dtype=torch.float64), none, 1.0, 8)
    with pytest.raises(ValueError):
        fl.secagg_mask_rows(torch.zeros(4, 6), none, 1.0, 8)
    with pytest.raises(ValueError, match="512"):
        fl.secagg_mask_rows(torch.zeros(513, 4), ([0] * 514, [], []), 1.0, 8)
    for entries in (([0, 0, 0, 0], [], []), ([0, 1, 1, 1, 1], [KEY], [2]), ([0, 1, 1, 1, 1], [2 ** 64], [1]),
                    ([0, 1, 1, 1, 2], [KEY], [1]), ([0, 1, 0, 1, 1], [KEY], [1]),
                    ([0, 513, 513, 513, 513], [KEY] * 513, [1] * 513)):
        with pytest.raises(ValueError):
            fl.secagg_mask_rows(x, entries, 1.0, 8)
    acc = torch.zeros(16, dtype=torch.int64)
    for rows in (torch.zeros(513, 16, dtype=torch.int32), torch.zeros(2, 12, dtype=torch.int32), torch.zeros(2, 16)):
        with pytest.raises(ValueError):
            fl.ring_sum(rows, acc)
    with pytest.raises(ValueError):
        fl.ring_sum(torch.zeros(2, 16, dtype=torch.int32), torch.zeros(16, dtype=torch.float64))
    with pytest.raises(ValueError):
        fl.ring_unmask(acc, ([KEY], [0]))
    assert not acc.any() and not x.any()  # nothing was written by a refused call


def test_in_place_upload_and_strided_rows_match_the_out_of_place_result():
    buf = _rows(3, 40, 4)
    x = buf[:, :32]  # row stride 40
    entries = ([0, 2, 2, 5], [KEY, 3, 4, 5, 6], [1, -1, 1, 1, -1])
    want, stats = fl.secagg_mask_rows(x.contiguous(), entries, 1.0, 20)
    keep = buf.clone()
    out = torch.full((3, 32), 7, dtype=torch.int32)
    got, _ = fl.secagg_mask_rows(x, entries, 1.0, 20, out=out)
    assert got is out and torch.equal(out, want) and torch.equal(buf, keep)  # inputs are read-only
    words, stats2 = fl.secagg_mask_rows(x, entries, 1.0, 20, out=x.view(torch.int32))
    assert torch.equal(words, want) and torch.equal(stats, stats2)
    assert torch.equal(buf[:, 32:], keep[:, 32:])  # the columns past P are untouched
    s = ref.secagg_mask_sum([KEY, 3], [1, -1], 32)
    assert s.tolist() == [_w(KEY, p) - _w(3, p) for p in range(32)]


def test_ring_sum_extremes_and_decode():
    rows = torch.tensor([[2 ** 31 - 1, -2 ** 31, 5, -5]] * 512, dtype=torch.int32)
    acc = torch.tensor([1, -1, 2 ** 40, 0], dtype=torch.int64)
    fl.ring_sum(rows, acc)
    assert acc.tolist() == [1 + 512 * (2 ** 31 - 1), -1 - 512 * 2 ** 31, 2 ** 40 + 2560, -2560]
    dec = fl.ring_decode(torch.tensor([2 ** 31, 2 ** 32 + 3, -1, 2 ** 31 - 1], dtype=torch.int64), 4)
    assert dec.tolist() == [-2 ** 31 / 16, 3 / 16, -1 / 16, (2 ** 31 - 1) / 16]
