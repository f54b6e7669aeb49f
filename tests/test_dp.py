"""The DP-FedAvg primitives on the CPU (`ops.fl.row_sq_norms`, `clip_scales`, `clipped_sum`,
`gaussian_add`; oracle ops/ref.py, kernels csrc/dp.hip): the contracts property by property. The
kernels are compared with the oracle in tests/test_dp_gpu.py."""

import functools
import math

import pytest
import torch

from distributed_learning_simulator_amd.ops import fl, ref

W, G = ref.PAIR_SPAN, ref.PAIR_GROUP
P3 = 2 * W + 48  # three spans, the last one ragged
PG = G * W + 48  # two groups: eight full spans, then a ragged one
DEN = 1e-40  # fp32 denormal
NAN, INF = float("nan"), float("inf")


def _bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _same(a, b):
    """Bitwise equal where not NaN, NaN at the same places (NaN payloads are not in the contract)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = a.isnan(), b.isnan()
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(_bits64(a)[~na], _bits64(b)[~nb])


def _dbits(v: float) -> int:
    return int(torch.tensor([v], dtype=torch.float64).view(torch.int64)[0])


def _wide(n, P, g):
    return torch.randn(n, P, generator=g) * torch.exp2(torch.randint(-60, 61, (n, P), generator=g).float())


@functools.lru_cache(maxsize=None)
def _data(kind: str, n: int, P: int) -> torch.Tensor:
    """The seven data kinds of tests/test_krum.py."""
    g = torch.Generator().manual_seed(1000 * n + P + 7 * len(kind))
    if kind == "gauss":
        x = torch.randn(n, P, generator=g)
    elif kind == "wide":
        x = _wide(n, P, g)
    elif kind == "ties":
        x = torch.randint(-8, 9, (n, P), generator=g).float() * 0.25
    elif kind == "equal":
        x = torch.randn(1, P, generator=g).repeat(n, 1)
    elif kind == "zeros":
        pool = torch.tensor([0.0, -0.0, DEN, -DEN, 1e-45, -1e-45])
        x = pool[torch.randint(0, len(pool), (n, P), generator=g)]
    elif kind == "special":  # NaN / ±inf / extreme values sprinkled over every row
        pool = torch.tensor([NAN, -NAN, INF, -INF, DEN, -DEN, 1e-45, -1e-45, 3e38, -3e38, 0.0, -0.0, 1.0, -1.0])
        x = torch.randn(n, P, generator=g)
        pick = torch.randint(0, 8 * len(pool), (n, P), generator=g)
        x = torch.where(pick < len(pool), pool[pick.clamp(max=len(pool) - 1)], x)
    elif kind == "poison":  # whole rows: NaN, +inf, −inf, alternating ±inf, huge
        x = torch.randn(n, P, generator=g)
        bad = [torch.full((P,), NAN), torch.full((P,), INF), torch.full((P,), -INF),
               torch.where(torch.arange(P) % 2 == 0, INF, -INF), torch.full((P,), 3e38)]
        for i in range(min(len(bad), n // 2)):
            x[2 * i] = bad[i]
    else:
        raise KeyError(kind)
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _norms(kind: str, n: int, P: int) -> torch.Tensor:
    """The CPU oracle's squared norms, computed once and shared (never modified)."""
    return ref.row_sq_norms(_data(kind, n, P))


def _restated_norm(a, descending=False):
    """Independent statement of the row_sq_norms contract for one row, with python floats (IEEE
    doubles): spans of W columns added sequentially from 0.0, groups of G span sums, the group sums."""
    P = len(a)
    spans = []
    for c0 in range(0, P, W):
        cols = range(c0, min(c0 + W, P))
        acc = 0.0
        for p in (reversed(cols) if descending else cols):
            acc += a[p] * a[p]
        spans.append(acc)
    total = 0.0
    for s0 in range(0, len(spans), G):
        group = 0.0
        for s in spans[s0 : s0 + G]:
            group += s
        total += group
    return total


# ------------------------------------------------------------------ Philox
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,expect", KAT)
def test_philox4x32_10_known_answers(counter, key, expect):
    got = ref.philox4x32(counter, key)
    assert " ".join(f"{int(w):08x}" for w in got) == expect
    # ... and as one element of a batch of counters
    c = [torch.tensor([5, v, 9], dtype=torch.int64) for v in counter]
    assert " ".join(f"{int(w[1]):08x}" for w in ref.philox4x32(c, key)) == expect


# ------------------------------------------------------------------ row_sq_norms
@pytest.mark.parametrize("P", [P3, PG])
def test_norm_summation_order_restated_with_python_floats(P):
    n = 5
    x = _data("wide", n, P)
    nsq = fl.row_sq_norms(x)
    assert nsq.dtype == torch.float64 and nsq.shape == (n,)
    for k in (0, 2, n - 1):
        assert _dbits(_restated_norm(x[k].tolist())) == int(_bits64(nsq)[k]), k


def test_norm_summation_order_is_observable():
    n = 13
    x, nsq = _data("wide", n, P3), _norms("wide", n, P3)
    differ = 0
    for k in range(n):
        row = x[k].tolist()
        assert _dbits(_restated_norm(row)) == int(_bits64(nsq)[k])
        differ += _dbits(_restated_norm(row, descending=True)) != int(_bits64(nsq)[k])
    print("rows whose descending-order sum differs:", differ, "of", n)
    assert differ >= 1


@pytest.mark.parametrize("kind", ["gauss", "wide", "zeros", "special"])
@pytest.mark.parametrize("P", [4112, P3])
def test_norm_has_the_bits_of_the_distance_to_a_zero_row(kind, P):
    x = _data(kind, 5, P)
    nsq = _norms(kind, 5, P)
    for k in range(5):
        D = fl.pairwise_sq_dists(torch.stack([x[k], torch.zeros(P)]))
        assert _same(D[0, 1], nsq[k]) and _same(D[1, 0], nsq[k])


def test_norm_strided_rows_and_zero_padding_columns_change_nothing():
    x, nsq = _data("wide", 7, P3), _norms("wide", 7, P3)
    for pad in (16, W - 48, W, G * W):
        assert torch.equal(_bits64(fl.row_sq_norms(torch.cat([x, torch.zeros(7, pad)], dim=1))), _bits64(nsq))
    wide = torch.full((7, P3 + 32), NAN)
    wide[:, 16 : 16 + P3] = x
    assert torch.equal(_bits64(fl.row_sq_norms(wide[:, 16 : 16 + P3])), _bits64(nsq))
    # nothing depends on n: a row alone, and `out` with guard values behind the n results
    assert torch.equal(_bits64(fl.row_sq_norms(x[3:4])), _bits64(nsq[3:4]))
    out = torch.full((9,), 7.0, dtype=torch.float64)
    assert fl.row_sq_norms(x, out=out) is out
    assert torch.equal(_bits64(out[:7]), _bits64(nsq)) and (out[7:] == 7).all()


def test_norm_counts_denormals():
    x = torch.zeros(2, 48)
    x[0, :5] = DEN
    x[1, 7] = 1e-45
    nsq = fl.row_sq_norms(x)
    d, t = float(torch.tensor(DEN)), float(torch.tensor(1e-45))
    assert float(nsq[0]) == d * d + d * d + d * d + d * d + d * d > 0.0
    assert float(nsq[1]) == t * t > 0.0
    assert (_norms("zeros", 13, 4112) > 0).all()


def test_norm_of_special_rows_is_not_finite():
    """NaN and ±inf rows give a non-finite squared norm. A row of 3e38 does NOT: its terms are 9e76 and
    even 2^30 of them stay far below the fp64 maximum 1.8e308, so no fp32 row of a size that fits in
    memory overflows the sum — such a row is finite, clipped like any large row, never rejected."""
    nsq = _norms("poison", 13, 4112)
    x = _data("poison", 13, 4112)
    assert nsq[0].isnan() and nsq[2] == INF and nsq[4] == INF and nsq[6] == INF
    assert torch.isfinite(nsq[[1, 3, 5, 7, 8, 9, 10, 11, 12]]).all()
    assert (x[8] == 3e38).all() and float(nsq[8]) == pytest.approx(4112 * 9e76, rel=1e-6)
    s, rej = fl.clip_scales(nsq, 1.0)
    assert rej.tolist() == [k in (0, 2, 4, 6) for k in range(13)] and 0.0 < float(s[8]) < 1e-39
    assert not torch.isfinite(_norms("special", 13, 4112)).any()  # NaN / inf sprinkled over every row


# ------------------------------------------------------------------ clip_scales
def test_clip_scales_rule():
    nsq = torch.tensor([0.0, 1.0, 4.0, 4.0 + 2.0 ** -50, 9.0, 1e300, 2.0 ** -1074, NAN, INF, -INF], dtype=torch.float64)
    s, rej = fl.clip_scales(nsq, 2.0)
    assert s.dtype == torch.float64 and rej.dtype == torch.bool
    assert rej.tolist() == [False] * 7 + [True] * 3
    assert s[:3].tolist() == [1.0, 1.0, 1.0]  # a zero row, norm < C, norm == C: exactly 1.0
    assert float(s[3]) == 2.0 / math.sqrt(4.0 + 2.0 ** -50)  # one ulp above C
    assert float(s[4]) == 2.0 / 3.0 and float(s[5]) == 2.0 / 1e150 and float(s[6]) == 1.0
    assert s[7:].tolist() == [0.0, 0.0, 0.0]


def test_clip_scales_bound_on_random_norms():
    g = torch.Generator().manual_seed(11)
    nsq = torch.exp2(torch.rand(4096, generator=g, dtype=torch.float64) * 200 - 100)
    for clip in (1e-3, 1.0, 37.5):
        s, rej = fl.clip_scales(nsq, clip)
        norm = torch.tensor([math.sqrt(v) for v in nsq.tolist()], dtype=torch.float64)  # correctly rounded
        assert not rej.any()
        assert (s[norm <= clip] == 1.0).all()
        big = norm > clip
        assert big.any() and s[big].tolist() == [clip / v for v in norm[big].tolist()]
        assert (s[big] * norm[big] <= clip * (1.0 + 2.0 ** -52)).all() and (s[big] < 1.0).all()


@pytest.mark.parametrize("clip", [0.0, -1.0, NAN, INF])
def test_clip_scales_rejects_bad_clip(clip):
    with pytest.raises(ValueError, match="clip"):
        fl.clip_scales(torch.ones(3, dtype=torch.float64), clip)
    with pytest.raises(ValueError, match="clip"):
        fl.clipped_sum(torch.ones(3, 16), torch.ones(3, dtype=torch.float64), clip)


def test_an_overflowed_square_sum_is_rejected():
    """What a finite row with an overflowing square sum would hand to clip_scales: +inf."""
    nsq = torch.tensor([1.7e308, 1.0], dtype=torch.float64) * 2.0
    assert nsq[0] == INF
    s, rej = fl.clip_scales(nsq, 1.0)
    assert rej.tolist() == [True, False] and s.tolist() == [0.0, 1.0 / math.sqrt(2.0)]


# ------------------------------------------------------------------ clipped_sum
def test_unclipped_rows_add_exactly_in_row_order():
    x = _data("wide", 13, 4112)
    nsq = _norms("wide", 13, 4112)
    got = fl.clipped_sum(x, nsq, 1e300)
    exp = torch.zeros(4112, dtype=torch.float64)
    for k in range(13):
        exp = exp + x[k].double()
    assert got.dtype == torch.float64 and torch.equal(_bits64(got), _bits64(exp))
    # the order is observable: descending rows give other bits somewhere
    rev = torch.zeros(4112, dtype=torch.float64)
    for k in reversed(range(13)):
        rev = rev + x[k].double()
    assert not torch.equal(_bits64(rev), _bits64(exp))


def test_clipped_sum_rounding_restated_with_python_floats():
    n, P = 7, 48
    x = _data("gauss", n, P)
    nsq = _norms("gauss", n, P)
    clip = float(nsq.sqrt().median())  # some rows clipped, some not
    s, _ = fl.clip_scales(nsq, clip)
    assert (s == 1.0).any() and (s < 1.0).any()
    start = torch.linspace(-3.0, 3.0, P, dtype=torch.float64)
    got = fl.clipped_sum(x, nsq, clip, out=start.clone())
    rows, sl = [r.tolist() for r in x], s.tolist()
    for p in range(P):
        acc = float(start[p])
        for k in range(n):
            t = sl[k] * rows[k][p]  # rounded once
            acc = acc + t  # rounded once more
        assert _dbits(acc) == int(_bits64(got)[p]), p


def test_clipped_sum_skips_rejected_rows_and_stays_finite():
    x = _data("poison", 13, 4112)
    nsq = _norms("poison", 13, 4112)
    s, rej = fl.clip_scales(nsq, 5.0)
    assert rej.tolist() == [k in (0, 2, 4, 6) for k in range(13)]
    got = fl.clipped_sum(x, nsq, 5.0)
    assert torch.isfinite(got).all()
    keep = [k for k in range(13) if k not in (0, 2, 4, 6)]
    assert torch.equal(_bits64(got), _bits64(fl.clipped_sum(x[keep].contiguous(), nsq[keep], 5.0)))
    # multiplying the rejected rows by their s = 0 instead would not: 0 · NaN, 0 · inf
    assert not torch.isfinite((x.double() * s[:, None]).sum(0)).all()


def test_clipped_sum_accumulates_in_place_across_calls():
    x = _data("gauss", 13, 4112)
    nsq = _norms("gauss", 13, 4112)
    clip = 60.0  # (norms ≈ sqrt(4112) = 64: most rows clipped)
    whole = fl.clipped_sum(x, nsq, clip)
    out = torch.full((4112 + 16,), 7.0, dtype=torch.float64)
    out[:4112] = 0.0
    assert fl.clipped_sum(x[:5], nsq[:5], clip, out=out) is out
    fl.clipped_sum(x[5:], nsq[5:], clip, out=out)
    assert torch.equal(_bits64(out[:4112]), _bits64(whole)) and (out[4112:] == 7).all()  # out[P:] untouched


@pytest.mark.parametrize("kind", ["gauss", "wide", "ties"])
def test_every_clipped_contribution_is_bounded_by_the_clip_norm(kind):
    x = _data(kind, 13, 4112)
    nsq = _norms(kind, 13, 4112)
    clip = float(nsq.sqrt().min()) * 0.5  # every row clipped
    for k in range(13):
        part = fl.clipped_sum(x[k : k + 1], nsq[k : k + 1], clip)
        assert float(part.square().sum().sqrt()) <= clip * (1.0 + 1e-12), k
        assert float(part.square().sum().sqrt()) >= clip * (1.0 - 1e-12), k


# ------------------------------------------------------------------ gaussian_add
SEED = 0x1234_5678_9ABC_DEF0


def test_noise_depends_on_seed_stream_and_position_only():
    z = ref.gaussian_noise(4112, SEED, 3)
    for start, n in ((0, 16), (1, 15), (7, 48), (1000, 1001), (4111, 1)):  # slices of the longer draw
        assert torch.equal(_bits64(ref.gaussian_noise(n, SEED, 3, start=start)), _bits64(z[start : start + n]))
    acc = torch.zeros(48, dtype=torch.float64)
    assert fl.gaussian_add(acc, 1.0, SEED, 3) is acc
    assert torch.equal(_bits64(acc), _bits64(z[:48]))
    other = [ref.gaussian_noise(48, SEED, 4), ref.gaussian_noise(48, SEED + 1, 3), ref.gaussian_noise(48, SEED ^ (1 << 40), 3)]
    for o in other:  # another stream, another low / high seed word
        assert not (o == z[:48]).any()
    # pair index past 2^32: the second counter word is used
    hi = ref.gaussian_noise(4, SEED, 3, start=2 ** 33)
    assert torch.isfinite(hi).all() and not torch.equal(hi, z[:4])


def test_noise_is_scaled_and_added_with_two_roundings():
    z = ref.gaussian_noise(48, SEED, 9)
    start = torch.linspace(-1.0, 1.0, 48, dtype=torch.float64)
    acc = fl.gaussian_add(start.clone(), 0.3, SEED, 9)
    for p in range(48):
        t = 0.3 * float(z[p])
        assert _dbits(float(start[p]) + t) == int(_bits64(acc)[p])


def test_masked_elements_are_untouched_bitwise_and_zero_std_changes_nothing():
    g = torch.Generator().manual_seed(5)
    start = torch.randn(4112, generator=g, dtype=torch.float64)
    start[::7] = -0.0
    start[3] = NAN
    mask = torch.rand(4112, generator=g) < 0.5
    for m in (mask, mask.to(torch.uint8)):
        acc = fl.gaussian_add(start.clone(), 2.0, SEED, 1, mask=m)
        assert torch.equal(_bits64(acc)[~mask], _bits64(start)[~mask])
        full = fl.gaussian_add(start.clone(), 2.0, SEED, 1)
        assert _same(acc[mask], full[mask]) and (acc[mask] != start[mask])[~start[mask].isnan()].all()
    same = fl.gaussian_add(start.clone(), 0.0, SEED, 1)
    assert torch.equal(_bits64(same), _bits64(start))  # (−0.0 stays −0.0: no draw is added at all)


def test_noise_moments_over_2_20_draws():
    N = 1 << 20
    z = ref.gaussian_noise(N, SEED, 1)
    mean = float(z.mean())
    var = float(((z - mean) ** 2).mean())
    kurt = float(((z - mean) ** 4).mean()) / var ** 2 - 3.0
    print("mean", mean, "var - 1", var - 1.0, "excess kurtosis", kurt, "max |z|", float(z.abs().max()))
    assert abs(mean) <= 5.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
    assert abs(kurt) <= 5.0 * math.sqrt(24.0 / N)
    assert float(z.abs().max()) <= 8.6
    # the two Box-Muller outputs of a pair are uncorrelated
    assert abs(float((z[0::2] * z[1::2]).mean())) <= 5.0 / math.sqrt(N / 2)
