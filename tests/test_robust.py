"""Coordinate-wise trimmed sum (`ops.fl.trimmed_sum`; oracle ops/ref.py, kernel csrc/robust.hip):
the contract property by property on the CPU, and the kernel against the oracle bit for bit on the
MI355X."""

import functools

import pytest
import torch

from distributed_learning_simulator_amd.ops import fl, ref


def _f32(bits: int) -> torch.Tensor:
    return torch.tensor([bits - (1 << 32) if bits >= (1 << 31) else bits], dtype=torch.int32).view(torch.float32)[0]


PNAN, NNAN = _f32(0x7FC00000), _f32(0xFFC00000)
DEN = 1e-40  # fp32 denormal
POISON = [PNAN, NNAN, torch.tensor(float("inf")), torch.tensor(float("-inf")), torch.tensor(3e38)]


def _bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _dbits(v) -> int:
    return int(torch.tensor([float(v)], dtype=torch.float64).view(torch.int64)[0])


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
    elif kind == "special":
        pool = torch.stack([PNAN, NNAN, *(torch.tensor(v) for v in (
            float("inf"), float("-inf"), DEN, -DEN, 1e-45, -1e-45, 3e38, -3e38, 0.0, -0.0, 1.0, -1.0))])
        x = torch.randn(n, P, generator=g)
        pick = torch.randint(0, 2 * len(pool), (n, P), generator=g)
        x = torch.where(pick < len(pool), pool[pick.clamp(max=len(pool) - 1)], x)
    elif kind == "poison":
        x = torch.randn(n, P, generator=g)
        for i in range(min(len(POISON), n)):
            x[i] = POISON[i]
    else:
        raise KeyError(kind)
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def _oracle(kind: str, n: int, P: int, b: int) -> torch.Tensor:
    """The CPU oracle's sums, computed once and shared (never modified)."""
    return ref.trimmed_sum(_data(kind, n, P), b)


def _ordered_sum(x, b, descending=False):
    """Independent statement of the contract: python-sorted keys, sequential fp64 adds."""
    n, P = x.shape
    order = torch.sort(ref.trim_keys(x), dim=0, descending=descending).indices
    rows = torch.gather(x, 0, order).double()
    acc = torch.zeros(P, dtype=torch.float64)
    for r in range(b, n - b):
        acc = acc + rows[r]
    return acc


# ------------------------------------------------------------------ oracle properties (CPU)
def test_b0_is_the_sequential_ascending_fp64_sum():
    x = _data("wide", 31, 48)
    got = fl.trimmed_sum(x, 0)
    assert got.dtype == torch.float64 and got.shape == (48,)
    assert torch.equal(_bits64(got), _bits64(_ordered_sum(x, 0)))
    # column by column with python floats (IEEE doubles), values sorted by the integer key
    keys = ref.trim_keys(x)
    for c in (0, 17, 47):
        acc = 0.0
        for _, v in sorted(zip(keys[:, c].tolist(), x[:, c].tolist())):
            acc += v
        assert _dbits(acc) == int(_bits64(got)[c])


@pytest.mark.parametrize("n", [1, 3, 5, 31, 129])
def test_median_of_odd_n_is_an_input_value_verbatim(n):
    x = _data("gauss", n, 48)
    got = fl.trimmed_sum(x, (n - 1) // 2)
    exp = x.sort(dim=0).values[n // 2].double()
    assert torch.equal(_bits64(got), _bits64(exp))
    assert torch.equal(got.float().view(torch.int32), x.sort(dim=0).values[n // 2].view(torch.int32))


@pytest.mark.parametrize("n", [2, 4, 64, 100])
def test_median_of_even_n_is_the_exact_mean_of_the_two_middle_values(n):
    x = _data("gauss", n, 48)
    got = fl.trimmed_sum(x, (n - 1) // 2) / 2.0
    s = x.sort(dim=0).values.double()
    assert torch.equal(_bits64(got), _bits64((s[n // 2 - 1] + s[n // 2]) / 2.0))


@pytest.mark.parametrize("kind", ["wide", "ties", "special"])
def test_row_permutations_give_bit_identical_output(kind):
    x = _data(kind, 31, 48)
    g = torch.Generator().manual_seed(3)
    for b in (0, 3, 15):
        base = _bits64(fl.trimmed_sum(x, b))
        for _ in range(3):
            perm = torch.randperm(31, generator=g)
            assert torch.equal(_bits64(fl.trimmed_sum(x[perm].contiguous(), b)), base)


def test_key_order_over_signed_zeros_denormals_infinities_and_nans():
    inf = float("inf")
    order = [NNAN, *(torch.tensor(v) for v in (-inf, -1.0, -DEN, -0.0, 0.0, DEN, 1.0, inf)), PNAN]
    vals = torch.stack(order)
    keys = ref.trim_keys(vals)
    assert keys.dtype == torch.int32 and (keys[1:] > keys[:-1]).all()
    # the key is an involution of the bits, and the median of any three neighbours is the middle one
    bits = vals.view(torch.int32)
    assert torch.equal(keys ^ ((keys >> 31) & 0x7FFFFFFF), bits)
    for i in range(1, len(order) - 1):
        col = torch.stack([order[i + 1], order[i - 1], order[i]]).reshape(3, 1).repeat(1, 16)
        got = fl.trimmed_sum(col, 1)
        # (the sum starts from +0.0, so a −0 median comes out as +0.0 + −0 = +0)
        assert torch.equal(_bits64(got), _bits64((0.0 + order[i].double()).repeat(16))), i
    # all ten, one of each: trimming the four lowest and highest leaves −0 + +0 (added from +0.0)
    col = vals[torch.tensor([3, 9, 0, 5, 7, 1, 8, 2, 6, 4])].reshape(10, 1).repeat(1, 16)
    assert torch.equal(_bits64(fl.trimmed_sum(col, 4)), torch.zeros(16, dtype=torch.int64))
    assert torch.equal(_bits64(fl.trimmed_sum(col, 3)), torch.zeros(16, dtype=torch.int64))  # −DEN + DEN
    # a NaN that survives the trim gives the canonical quiet NaN
    assert (_bits64(fl.trimmed_sum(col, 0)) == 0x7FF8000000000000).all()


def test_invalid_trim_and_too_many_rows_raise():
    x = torch.zeros(4, 16)
    for b in (2, 3, -1):
        with pytest.raises(ValueError):
            fl.trimmed_sum(x, b)
    with pytest.raises(ValueError):
        fl.trimmed_sum(torch.zeros(1, 16), 1)
    with pytest.raises(ValueError, match="512"):
        fl.trimmed_sum(torch.zeros(513, 16), 0)
    fl.trimmed_sum(torch.zeros(512, 16), 255)


def test_oversized_out_keeps_its_tail():
    x = _data("gauss", 5, 48)
    out = torch.full((64,), 7.0, dtype=torch.float64)
    assert fl.trimmed_sum(x, 1, out=out) is out
    assert torch.equal(_bits64(out[:48]), _bits64(_oracle("gauss", 5, 48, 1))) and (out[48:] == 7).all()


def test_summation_order_is_observable():
    """The GPU comparison below can only pass with ascending adds: on the wide-exponent input the
    descending-order sum differs from the contract's in many columns."""
    x = _data("wide", 100, 4112)
    asc = _oracle("wide", 100, 4112, 10)
    assert torch.equal(_bits64(asc), _bits64(_ordered_sum(x, 10)))
    differ = int((_bits64(asc) != _bits64(_ordered_sum(x, 10, descending=True))).sum())
    print("columns whose descending-order sum differs:", differ, "of 4112")
    assert differ >= 1


def test_poisoned_rows_cannot_move_the_result_outside_the_honest_range():
    g = torch.Generator().manual_seed(11)
    honest = torch.randn(20, 4112, generator=g)
    x = torch.cat([honest, torch.stack(POISON)[:, None].expand(5, 4112)])[torch.randperm(25, generator=g)]
    for b in (5, 8, 12):
        mean = fl.trimmed_sum(x.contiguous(), b) / (25 - 2 * b)
        assert torch.isfinite(mean).all()
        assert (mean >= honest.double().min(0).values).all() and (mean <= honest.double().max(0).values).all()
    assert not torch.isfinite(fl.trimmed_sum(x.contiguous(), 1)).all()  # ±inf survive a trim of one


# ------------------------------------------------------------------ HIP kernel vs the oracle
NS = [1, 2, 3, 4, 5, 31, 63, 64, 65, 100, 128, 129, 512]
PS = [16, 48, 4112]
KINDS = ["gauss", "wide", "ties", "equal", "zeros", "special", "poison"]


def _trims(n):
    return sorted({0, 1, n // 10, (n - 1) // 2})


# the only combinations of the grid that are not run: 2b ≥ n is not a trimmed sum
SKIPPED = [(n, b) for n in NS for b in _trims(n) if 2 * b >= n]
assert SKIPPED == [(1, 1), (2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_hip_trimmed_sum_matches_oracle_bit_for_bit(hip, n, kind):
    """fp64 sums compared as int64. A NaN sum is the canonical quiet NaN on both sides, so columns
    whose kept values are all NaN (or whose sum is inf − inf) compare by bits as well, which
    includes their NaN-ness."""
    for P in PS:
        xc = _data(kind, n, P)
        wide = torch.full((n, P + 48), float("nan"), device="cuda")  # rows as a view, ld > P
        wide[:, 16 : 16 + P] = xc.cuda()
        for x in (xc.cuda(), wide[:, 16 : 16 + P]):
            for b in _trims(n):
                if (n, b) in SKIPPED:
                    continue
                got = fl.trimmed_sum(x, b)
                assert got.dtype == torch.float64 and got.shape == (P,)
                exp = _oracle(kind, n, P, b)
                same = _bits64(got) == _bits64(exp)
                assert same.all(), (n, P, b, kind, x.stride(0), int((~same).sum()), got.cpu()[~same][:4],
                                    exp[~same][:4])
                assert torch.equal(got.isnan().cpu(), exp.isnan())


@pytest.mark.gpu
def test_hip_trimmed_sum_is_reproducible_and_respects_out(hip):
    x = _data("wide", 100, 4112).cuda()
    a, b2 = fl.trimmed_sum(x, 10), fl.trimmed_sum(x, 10)
    assert torch.equal(_bits64(a), _bits64(b2))
    out = torch.full((4112 + 64,), 7.0, dtype=torch.float64, device="cuda")  # guard values past P
    assert fl.trimmed_sum(x, 10, out=out) is out
    assert torch.equal(_bits64(out[:4112]), _bits64(_oracle("wide", 100, 4112, 10))) and (out[4112:] == 7).all()
    small = torch.full((32,), 7.0, dtype=torch.float64, device="cuda")
    fl.trimmed_sum(_data("gauss", 5, 16).cuda(), 1, out=small)
    assert torch.equal(_bits64(small[:16]), _bits64(_oracle("gauss", 5, 16, 1))) and (small[16:] == 7).all()


@pytest.mark.gpu
def test_hip_trimmed_sum_rejects_bad_arguments(hip):
    with pytest.raises(ValueError, match="512"):
        fl.trimmed_sum(torch.zeros(513, 16, device="cuda"), 0)
    with pytest.raises(ValueError):
        fl.trimmed_sum(torch.zeros(4, 16, device="cuda"), 2)
