"""Pairwise squared distances and the Krum selection (`ops.fl.pairwise_sq_dists`, `ops.fl.krum_select`;
oracle ops/ref.py, kernel csrc/krum.hip): the contract property by property on the CPU, and the
kernel against the oracle bit for bit on the MI355X."""

import functools
import itertools

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


def _wide(n, P, g):
    return torch.randn(n, P, generator=g) * torch.exp2(torch.randint(-60, 61, (n, P), generator=g).float())


@functools.lru_cache(maxsize=None)
def _data(kind: str, n: int, P: int) -> torch.Tensor:
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
def _oracle(kind: str, n: int, P: int) -> torch.Tensor:
    """The CPU oracle's distances, computed once and shared (never modified)."""
    return ref.pairwise_sq_dists(_data(kind, n, P))


def _restated(a, b, descending=False):
    """Independent statement of the contract for one pair of rows, with python floats (IEEE doubles):
    spans of W columns added sequentially from 0.0, groups of G span sums, then the group sums."""
    P = len(a)
    spans = []
    for c0 in range(0, P, W):
        cols = range(c0, min(c0 + W, P))
        acc = 0.0
        for p in (reversed(cols) if descending else cols):
            d = a[p] - b[p]
            acc += d * d
        spans.append(acc)
    total = 0.0
    for s0 in range(0, len(spans), G):
        group = 0.0
        for s in spans[s0 : s0 + G]:
            group += s
        total += group
    return total


def _dbits(v: float) -> int:
    return int(torch.tensor([v], dtype=torch.float64).view(torch.int64)[0])


# ------------------------------------------------------------------ oracle properties (CPU)
@pytest.mark.parametrize("P", [P3, PG])
def test_summation_order_restated_with_python_floats(P):
    n = 13 if P == P3 else 5
    x = _data("wide", n, P)
    D = fl.pairwise_sq_dists(x)
    assert D.dtype == torch.float64 and D.shape == (n, n)
    rows = [r.tolist() for r in x]  # fp32 values as exact doubles
    for i, j in ((0, 1), (n - 1, 2), (3, n - 2)):
        assert _dbits(_restated(rows[i], rows[j])) == int(_bits64(D)[i, j]), (i, j)


def test_summation_order_is_observable():
    """The same terms added in plain descending column order give other bits on wide-exponent data:
    a comparison against the oracle can see the order."""
    n = 13
    x, D = _data("wide", n, P3), _oracle("wide", n, P3)
    rows = [r.tolist() for r in x]
    differ = 0
    for i, j in itertools.combinations(range(0, n, 3), 2):
        assert _dbits(_restated(rows[i], rows[j])) == int(_bits64(D)[i, j])
        differ += _dbits(_restated(rows[i], rows[j], descending=True)) != int(_bits64(D)[i, j])
    print("pairs whose descending-order sum differs:", differ, "of 10")
    assert differ >= 1


def _fma_cases():
    """[2, 16] inputs whose first column gives the term t = 2^-54 and whose second column's product
    d · d ≈ 1 is inexact in fp64 (t is a quarter of its last place): (x, the contract's value
    fl(t + fl(d · d)), whether a fused multiply-add fl(t + d · d) would give other bits)."""
    from fractions import Fraction

    cases, t = [], 2.0 ** -54
    for k in range(32):
        x = torch.zeros(2, 16)
        x[0, 0] = 2.0 ** -27
        m = (2654435761 * (k + 1)) % (1 << 23) | 1
        x[0, 1], x[1, 1] = 1.0 + (2 * m + 1) % (1 << 22) * 2.0 ** -23, 2.0 ** -29 * (1.0 + m * 2.0 ** -23)
        d = float(x[0, 1]) - float(x[1, 1])  # exact: 53 significant bits
        cases.append((x, t + d * d, float(Fraction(t) + Fraction(d) ** 2) != t + d * d))
    return cases


def test_multiply_and_add_are_rounded_separately():
    cases = _fma_cases()
    assert sum(differs for _, _, differs in cases) >= 1  # the inputs can tell an FMA from mul + add
    for x, two_roundings, _ in cases:
        D = fl.pairwise_sq_dists(x)
        assert float(D[0, 1]) == two_roundings == float(D[1, 0])


@pytest.mark.parametrize("kind", ["gauss", "wide", "ties", "zeros"])
def test_zero_diagonal_and_bitwise_symmetry(kind):
    D = _oracle(kind, 13, P3)
    assert (_bits64(D.diagonal()) == 0).all()  # +0.0, not −0.0
    assert torch.equal(_bits64(D), _bits64(D.t()))
    assert torch.isfinite(D).all() and (D >= 0).all()


@pytest.mark.parametrize("kind", ["wide", "ties", "special"])
def test_row_permutation_permutes_D_bitwise(kind):
    x, D = _data(kind, 13, P3), _oracle(kind, 13, P3)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        perm = torch.randperm(13, generator=g)
        assert _same(fl.pairwise_sq_dists(x[perm].contiguous()), D[perm][:, perm])


def test_zero_padding_columns_change_nothing():
    x, D = _data("wide", 7, P3), _oracle("wide", 7, P3)
    for pad in (16, W - 48, W, G * W):
        assert torch.equal(_bits64(fl.pairwise_sq_dists(torch.cat([x, torch.zeros(7, pad)], dim=1))), _bits64(D))
    # ... and strided rows (a view of a wider buffer) are the same rows
    wide = torch.full((7, P3 + 32), NAN)
    wide[:, 16 : 16 + P3] = x
    assert torch.equal(_bits64(fl.pairwise_sq_dists(wide[:, 16 : 16 + P3])), _bits64(D))


def test_equal_rows_single_row_and_too_many_rows():
    assert (_bits64(_oracle("equal", 13, P3)) == 0).all()
    one = fl.pairwise_sq_dists(_data("gauss", 1, 48))
    assert one.shape == (1, 1) and int(_bits64(one)[0, 0]) == 0
    with pytest.raises(ValueError, match="512"):
        fl.pairwise_sq_dists(torch.zeros(513, 16))
    assert fl.pairwise_sq_dists(torch.zeros(512, 16)).shape == (512, 512)
    out = torch.full((3, 3), 7.0, dtype=torch.float64)
    assert fl.pairwise_sq_dists(_data("gauss", 3, 48), out=out) is out
    assert torch.equal(_bits64(out), _bits64(_oracle("gauss", 3, 48)))


def test_special_rows_poison_exactly_their_rows_and_columns():
    n = 13
    x, D = _data("poison", n, 4112), _oracle("poison", n, 4112)
    bad = ~torch.isfinite(x).all(dim=1)
    # (row 8, all 3e38, is finite: its distances are large, ≈ 4112 · 9e76, but finite)
    assert bad.tolist() == [i in (0, 2, 4, 6) for i in range(n)]
    expect_bad = bad[:, None] | bad[None, :]
    assert torch.equal(~torch.isfinite(D), expect_bad)
    assert (D[~expect_bad] >= 0).all()
    assert D[0].isnan().all() and D[:, 0].isnan().all()  # NaN row
    assert D[2, 1] == INF and D[2, 4] == INF and D[2, 2].isnan()  # inf − finite, inf − (−inf), inf − inf
    assert D[6, 2].isnan()  # (±inf alternating) − (+inf): inf − inf in every other column


# ------------------------------------------------------------------ krum_select (CPU)
def _brute(D, f, m, ids):
    """Brute-force Krum selection on python lists."""
    n = len(ids)
    if n < 2 * f + 3:
        f = max(0, (n - 3) // 2)
    k = min(max(n - f - 2, 1), n - 1)
    scores = []
    for i in range(n):
        others = sorted(INF if (v != v or v in (INF, -INF)) else v for j, v in enumerate(D[i]) if j != i)
        s = 0.0
        for v in others[:k]:
            s += v
        scores.append(s if n > 1 else 0.0)
    m = min(max(m, 1), n)
    best = sorted(range(n), key=lambda i: (scores[i], ids[i]))[:m]
    return sorted(best, key=lambda i: ids[i]), scores


def _rand_D(n, g):
    x = torch.randn(n, 64, generator=g)
    return ref.pairwise_sq_dists(x)


@pytest.mark.parametrize("n,f,m", [(1, 0, 1), (2, 0, 1), (3, 0, 2), (7, 2, 1), (7, 2, 5), (13, 4, 9), (13, 0, 13),
                                   (20, 5, 3)])
def test_krum_select_equals_brute_force(n, f, m):
    g = torch.Generator().manual_seed(n * 100 + f * 10 + m)
    for _ in range(3):
        D = _rand_D(n, g)
        ids = torch.randperm(100, generator=g)[:n].tolist()
        sel, scores = _brute(D.tolist(), f, m, ids)
        assert fl.krum_select(D, f, m, ids) == sel
        got, f_used = fl.krum_scores(D, f)
        assert got.tolist() == scores and f_used == f
        assert [ids[i] for i in sel] == sorted(ids[i] for i in sel) and len(sel) == m


def test_krum_select_ties_are_resolved_by_client_id():
    D = torch.zeros(5, 5, dtype=torch.float64)  # every score equal
    ids = [40, 7, 23, 3, 11]
    assert fl.krum_select(D, 1, 1, ids) == [3]
    assert fl.krum_select(D, 1, 2, ids) == [3, 1]  # the rows of ids 3 and 7, in client-id order
    assert fl.krum_select(D, 1, 3, ids) == [3, 1, 4]
    # two pairs of twins: all four scores are equal (0 + 400), the lowest id wins
    x = torch.zeros(4, 16)
    x[2:] = 5.0
    D = ref.pairwise_sq_dists(x)
    assert fl.krum_select(D, 0, 1, [9, 8, 1, 0]) == [3]
    assert fl.krum_select(D, 0, 1, [9, 8, 0, 1]) == [2]


def test_krum_select_is_invariant_under_row_permutation_with_ids():
    g = torch.Generator().manual_seed(17)
    x = torch.randint(-2, 3, (11, 32), generator=g).float()  # many tied distances
    ids = torch.randperm(50, generator=g)[:11].tolist()
    D = ref.pairwise_sq_dists(x)
    for m in (1, 4, 8):
        base = sorted(ids[i] for i in fl.krum_select(D, 3, m, ids))
        for _ in range(3):
            perm = torch.randperm(11, generator=g)
            Dp = ref.pairwise_sq_dists(x[perm].contiguous())
            idp = [ids[i] for i in perm.tolist()]
            assert sorted(idp[i] for i in fl.krum_select(Dp, 3, m, idp)) == base


@pytest.mark.parametrize("n,f", [(5, 1), (7, 2), (13, 5), (20, 4)])
def test_poisoned_rows_are_never_selected(n, f):
    g = torch.Generator().manual_seed(n + f)
    x = torch.randn(n, 256, generator=g)
    poison = [torch.full((256,), NAN), torch.full((256,), INF), x[n - 1] * 1e6, torch.full((256,), -INF),
              torch.randn(256, generator=g) * 1e6]
    bad = torch.randperm(n, generator=g)[:f].tolist()
    for k, i in enumerate(bad):
        x[i] = poison[k % len(poison)]
    D = ref.pairwise_sq_dists(x)
    ids = list(range(100, 100 + n))
    for m in (1, n - f):
        sel = fl.krum_select(D, f, m, ids)
        assert len(sel) == m and not set(sel) & set(bad), (sel, bad)


def test_krum_fallback_for_small_rounds_and_m_is_clamped():
    g = torch.Generator().manual_seed(2)
    D = _rand_D(4, g)
    ids = [3, 1, 2, 0]
    scores, f_used = fl.krum_scores(D, 3)  # 4 < 2·3 + 3: f' = (4 − 3) // 2 = 0
    assert f_used == 0 and scores.tolist() == _brute(D.tolist(), 0, 1, ids)[1]
    assert fl.krum_select(D, 3, 1, ids) == _brute(D.tolist(), 3, 1, ids)[0] == fl.krum_select(D, 0, 1, ids)
    assert fl.krum_scores(_rand_D(6, g), 2)[1] == 1  # 6 < 7: f' = 1
    assert fl.krum_scores(_rand_D(2, g), 1)[1] == 0
    assert fl.krum_select(D, 0, 0, ids) == fl.krum_select(D, 0, 1, ids)  # m < 1 -> 1
    assert fl.krum_select(D, 0, 99, ids) == [3, 1, 2, 0]  # m > n -> n, in client-id order
    assert fl.krum_select(torch.zeros(1, 1, dtype=torch.float64), 5, 3, [42]) == [0]


# ------------------------------------------------------------------ HIP kernel vs the oracle
# n: one row, a partial register block (1, 2, 3), a partial row block (13 of 16, 17 of 32), whole
# blocks (32, 64), one more row than a block (17, 33, 65), several tiles with a partial last block
# (100), the largest cohort (512)
NS = [1, 2, 3, 13, 17, 32, 33, 64, 65, 100, 512]
PS = [16, 48, 4112]
KINDS = ["gauss", "wide", "ties", "equal", "zeros", "special", "poison"]


def _strided(xc):
    """The rows as a view of a wider buffer (ld > P) with NaN guard values between the rows."""
    n, P = xc.shape
    wide = torch.full((n, P + 48), NAN, device="cuda")
    wide[:, 16 : 16 + P] = xc.cuda()
    return wide[:, 16 : 16 + P]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_hip_pairwise_matches_oracle_bit_for_bit(hip, n, kind):
    for P in PS:
        xc, exp = _data(kind, n, P), _oracle(kind, n, P)
        for x in (xc.cuda(), _strided(xc)):
            got = fl.pairwise_sq_dists(x)
            assert got.dtype == torch.float64 and got.shape == (n, n) and got.is_cuda
            assert _same(got, exp), (n, P, kind, x.stride(0), int((_bits64(got) != _bits64(exp)).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wide", "special"])
@pytest.mark.parametrize("n,P", [(3, P3), (13, P3), (13, PG), (17, PG), (65, PG)])
def test_hip_pairwise_folds_spans_and_groups_like_the_oracle(hip, n, P, kind):
    """Ragged last span, the fold across spans and across groups — with a workgroup per span and
    with a workgroup per group of spans (the launch geometry changes no bit)."""
    xc, exp = _data(kind, n, P), _oracle(kind, n, P)
    for x in (xc.cuda(), _strided(xc)):
        for spw in (None, 1, G):
            got = hip.pairwise_sq_dists(x, spans_per_wg=spw)
            assert _same(got, exp), (n, P, kind, spw, x.stride(0))


@pytest.mark.gpu
def test_hip_pairwise_leaves_guard_values_untouched_and_is_reproducible(hip):
    for n, P, spw in ((13, P3, 1), (65, PG, G), (100, 4112, 1)):
        x = _data("wide", n, P).cuda()
        need = hip.pairwise_scratch_doubles(n, P, spw)
        buf = torch.full((64 + need + 64,), 7.0, dtype=torch.float64, device="cuda")  # scratch with neighbours
        res = torch.full((n * n + 64,), 7.0, dtype=torch.float64, device="cuda")  # guard values past [n, n]
        out = res[: n * n].view(n, n)
        assert hip.pairwise_sq_dists(x, out=out, scratch=buf[64 : 64 + need], spans_per_wg=spw) is out
        assert (buf[:64] == 7).all() and (buf[64 + need :] == 7).all() and (res[n * n :] == 7).all()
        assert _same(out, _oracle("wide", n, P))
        again = fl.pairwise_sq_dists(x)
        assert torch.equal(_bits64(again), _bits64(out))  # two launches, other scratch: the same bits
        # symmetry and the zero diagonal on the device result itself
        assert torch.equal(_bits64(out), _bits64(out.t())) and (_bits64(out.diagonal()) == 0).all()


@pytest.mark.gpu
def test_hip_pairwise_rounds_multiply_and_add_separately(hip):
    for x, two_roundings, _ in _fma_cases():
        D = fl.pairwise_sq_dists(x.cuda()).cpu()
        assert float(D[0, 1]) == two_roundings == float(D[1, 0])


@pytest.mark.gpu
def test_hip_pairwise_rejects_too_many_rows(hip):
    with pytest.raises(ValueError, match="512"):
        fl.pairwise_sq_dists(torch.zeros(513, 16, device="cuda"))
