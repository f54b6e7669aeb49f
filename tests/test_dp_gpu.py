"""The DP-FedAvg kernels (csrc/dp.hip) against the CPU oracle (ops/ref.py) on the MI355X: squared
norms and the clipped sum bit for bit, the Gaussian draw within the libm bound of the contract
(`ops.fl.gaussian_add`), and one `fed_dp_avg` session against the oracle on its own uploads."""

import functools
import os
import sys

import pytest
import torch

from distributed_learning_simulator_amd.ops import fl, ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dp as TDP  # noqa: E402  (data kinds, the shared oracle norms, the bitwise helpers)
import test_dp_sessions as TS  # noqa: E402  (session helpers and spies)

pytestmark = pytest.mark.gpu

W, G, P3, PG, NAN = TDP.W, TDP.G, TDP.P3, TDP.PG, TDP.NAN
_bits64, _same, _data, _norms = TDP._bits64, TDP._same, TDP._data, TDP._norms

# n: one row, a few, a partial wave of rows, several workgroups of rows; P: one quad of columns, less
# than a stage, one span and a ragged second, three spans (ragged), two groups of spans (ragged)
NS = [1, 2, 3, 13, 64, 65, 100]
PS = [16, 48, 4112, P3, PG]
KINDS = ["gauss", "wide", "ties", "equal", "zeros", "special", "poison"]


def _strided(xc):
    """The rows as a view of a wider buffer (ld > P) with NaN guard values between the rows."""
    n, P = xc.shape
    wide = torch.full((n, P + 48), NAN, device="cuda")
    wide[:, 16 : 16 + P] = xc.cuda()
    return wide[:, 16 : 16 + P]


def _clips(nsq):
    """Clip norms below, between and above the rows' finite, positive norms (1.0 if there is none)."""
    norm = nsq.sqrt()
    norm = norm[torch.isfinite(norm) & (norm > 0)]
    if norm.numel() == 0:
        return [1.0]
    return [float(norm.min()) * 0.5, float(norm.median()), float(norm.max()) * 2.0]


@functools.lru_cache(maxsize=None)
def _start(P: int) -> torch.Tensor:
    return torch.randn(P, generator=torch.Generator().manual_seed(P), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _clipped(kind: str, n: int, P: int):
    """[(clip, the oracle's clipped sum accumulated into `_start(P)`)], computed once and shared."""
    x, nsq = _data(kind, n, P), _norms(kind, n, P)
    return [(c, ref.clipped_sum(x, nsq, c, out=_start(P).clone())) for c in _clips(nsq)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_hip_norms_and_clipped_sum_match_oracle_bit_for_bit(hip, n, kind):
    for P in PS:
        xc, exp = _data(kind, n, P), _norms(kind, n, P)
        for x in (xc.cuda(), _strided(xc)):
            nsq = fl.row_sq_norms(x)
            assert nsq.dtype == torch.float64 and nsq.shape == (n,) and nsq.is_cuda
            assert _same(nsq, exp), (n, P, kind, x.stride(0), int((_bits64(nsq) != _bits64(exp)).sum()))
            s_exp, rej_exp = ref.clip_scales(exp, _clips(exp)[-1] * 0.75)
            s, rej = fl.clip_scales(nsq, _clips(exp)[-1] * 0.75)
            assert s.is_cuda and torch.equal(rej.cpu(), rej_exp) and torch.equal(_bits64(s), _bits64(s_exp))
            for clip, want in _clipped(kind, n, P):
                out = _start(P).cuda()  # accumulating into a non-zero `out`
                assert fl.clipped_sum(x, nsq, clip, out=out) is out
                assert _same(out, want), (n, P, kind, clip, x.stride(0), int((_bits64(out) != _bits64(want)).sum()))


def test_hip_guard_values_inputs_and_reproducibility(hip):
    for n, P in ((13, P3), (65, PG), (100, 4112), (3, 16)):
        xc = _data("wide", n, P)
        x = _strided(xc)
        base = x._base.clone()
        need = hip.row_sq_norms_scratch_doubles(n, P)
        assert need == n * ((P + W - 1) // W)
        buf = torch.full((64 + need + 64,), 7.0, dtype=torch.float64, device="cuda")  # scratch with neighbours
        res = torch.full((n + 64,), 7.0, dtype=torch.float64, device="cuda")  # guard values past [n]
        assert hip.row_sq_norms(x, out=res, scratch=buf[64 : 64 + need]) is res
        assert (buf[:64] == 7).all() and (buf[64 + need :] == 7).all() and (res[n:] == 7).all()
        assert _same(res[:n], _norms("wide", n, P))
        nsq = res[:n].clone()
        again = fl.row_sq_norms(x)  # two launches, other scratch: the same bits
        assert torch.equal(_bits64(again), _bits64(nsq))
        clip, want = _clipped("wide", n, P)[1]
        out = torch.full((P + 64,), 7.0, dtype=torch.float64, device="cuda")
        out[:P] = _start(P).cuda()
        fl.clipped_sum(x, nsq, clip, out=out)
        assert (out[P:] == 7).all() and _same(out[:P], want)  # out[P:] untouched
        twice = _start(P).cuda()
        fl.clipped_sum(x, nsq, clip, out=twice)
        assert torch.equal(_bits64(twice), _bits64(out[:P]))
        # x (guard columns between the rows included) and nsq are read-only
        assert torch.equal(x._base.view(torch.int32), base.view(torch.int32))
        assert torch.equal(_bits64(nsq), _bits64(res[:n]))


def test_hip_clipped_sum_over_waves_equals_one_call(hip):
    n, P = 65, PG
    x, nsq = _data("gauss", n, P).cuda(), _norms("gauss", n, P).cuda()
    clip = float(_norms("gauss", n, P).sqrt().median())
    whole = fl.clipped_sum(x, nsq, clip)
    out = torch.zeros(P, dtype=torch.float64, device="cuda")
    for a, b in ((0, 13), (13, 14), (14, 65)):
        fl.clipped_sum(x[a:b], nsq[a:b], clip, out=out)
    assert torch.equal(_bits64(out), _bits64(whole))
    assert _same(whole, ref.clipped_sum(_data("gauss", n, P), _norms("gauss", n, P), clip))


SEED = 0x1234_5678_9ABC_DEF0


@functools.lru_cache(maxsize=None)
def _noise(P: int) -> torch.Tensor:
    return ref.gaussian_noise(P, SEED, 7)


@pytest.mark.parametrize("P", [16, 48, 4111, 4112, (1 << 20) + 48])
def test_hip_gaussian_add_matches_oracle_within_the_libm_bound(hip, P):
    g = torch.Generator().manual_seed(P)
    start = torch.randn(P, generator=g, dtype=torch.float64) * 3.0
    start[::5] = -0.0
    mask = torch.rand(P, generator=g) < 0.6
    z = _noise(P)
    for std in (1.0, 0.37e-3):
        for m in (None, mask):
            acc = start.cuda()
            assert fl.gaussian_add(acc, std, SEED, 7, None if m is None else m.cuda()) is acc
            want = ref.gaussian_add(start.clone(), std, SEED, 7, m)
            err = (acc.cpu() - want).abs()
            bound = std * 1e-13 + 2.0 ** -52 * want.abs()
            print("P", P, "std", std, "masked", m is not None, "max err / std", float(err.max()) / std)
            assert (err <= bound).all(), (P, std, float((err - bound).max()))
            if m is not None:  # masked elements bitwise untouched
                assert torch.equal(_bits64(acc)[~m], _bits64(start)[~m])
                assert (acc.cpu()[m] != start[m]).all()
            else:  # ... and z itself, from a zero accumulator
                zg = fl.gaussian_add(torch.zeros(P, dtype=torch.float64, device="cuda"), 1.0, SEED, 7).cpu()
                assert float((zg - z).abs().max()) <= 1e-13
    # another stream gives another draw; two launches the same bits
    a = fl.gaussian_add(torch.zeros(P, dtype=torch.float64, device="cuda"), 1.0, SEED, 8)
    b = fl.gaussian_add(torch.zeros(P, dtype=torch.float64, device="cuda"), 1.0, SEED, 8)
    assert torch.equal(_bits64(a), _bits64(b)) and not (a.cpu() == z).any()
    same = fl.gaussian_add(start.cuda(), 0.0, SEED, 7)
    assert torch.equal(_bits64(same), _bits64(start))


def test_hip_gaussian_add_does_not_depend_on_the_position_in_the_buffer(hip):
    """z depends on (seed, stream, p) alone: a draw over a prefix equals the prefix of a longer draw."""
    long = fl.gaussian_add(torch.zeros(4112, dtype=torch.float64, device="cuda"), 1.0, SEED, 2)
    for P in (2, 16, 1001):
        short = fl.gaussian_add(torch.zeros(P, dtype=torch.float64, device="cuda"), 1.0, SEED, 2)
        assert torch.equal(_bits64(short), _bits64(long[:P]))


GPU = {"round": 2, "worker_number": 5, "dataset_kwargs.scale": 0.02, "save_models": False,
       "algorithm_kwargs.byzantine_number": 1}


@pytest.mark.parametrize("z", [0.0, 0.8])
def test_gpu_session_equals_oracle_on_its_uploads(hip, tmp_path, monkeypatch, z):
    """The rows a GPU session uploaded, copied to the CPU and run through the oracle: with the noise
    off the new θ bit for bit, with it on within the libm bound scaled by z · C / m."""
    rounds, uploads = [], []
    TS._spy_rounds(monkeypatch, rounds)
    TS._spy_uploads(monkeypatch, uploads)
    clip = 0.009
    ov = {**GPU, "algorithm_kwargs.dp_clip_norm": clip, "algorithm_kwargs.dp_noise_multiplier": z}
    sess, _ = TS._run(ov, tmp_path / "a", "cuda")
    assert len(rounds) == 2 and rounds[0]["acc"].is_cuda
    valid = sess.layout.valid_mask()
    for r, up in zip(rounds, TS._uploads_by_round(uploads, rounds)):
        assert r["n"] == 5 and r["clipped"] >= 1
        exp, noise_scale = TS._oracle_round(r, up, clip, z, m=5, seed=sess.config.seed, valid=valid)
        got = r["new64"].cpu()
        if z == 0.0:
            assert torch.equal(_bits64(got), _bits64(exp))
        else:
            # the accumulator after the noise: the bound of gaussian_add with std = z · C (dividing
            # both sides by m gives the bound on the mean, whose noise std is z · C / m) ...
            want, _ = TS._oracle_acc(up, clip)
            ref.gaussian_add(want, z * clip, sess.config.seed, r["round"], valid)
            err = (r["acc"].cpu() - want).abs()
            print("max err / (z C):", float(err.max()) / (z * clip), "noise std on the mean:", noise_scale)
            assert (err <= z * clip * 1e-13 + 2.0 ** -52 * want.abs()).all()
            assert torch.equal(_bits64(r["acc"].cpu()[~valid]), _bits64(want[~valid]))  # no noise on the padding
            # ... and θ_{t+1} = θ_t + acc / m exactly, from the kernel's own accumulator
            assert torch.equal(_bits64(got), _bits64(r["old"].cpu().double() + r["acc"].cpu() / 5.0))
        assert torch.equal(r["new"].cpu(), got.float())
    assert torch.isfinite(sess.server.global_parameter).all()
    assert (sess.server.global_parameter.cpu()[~valid].view(torch.int32) == 0).all()  # padding stays +0
