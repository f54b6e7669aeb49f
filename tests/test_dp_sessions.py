"""fed_dp_avg sessions: client-level DP-FedAvg as a registered method (method/fed_dp_avg,
algorithm/dp_algorithm, worker/robust_worker.ByzantineWorker, utils/privacy)."""

import math
import os
import sys
import types

import pytest
import torch

from distributed_learning_simulator_amd.algorithm import dp_algorithm as DA
from distributed_learning_simulator_amd.config import load_config
from distributed_learning_simulator_amd.message import CohortMessage
from distributed_learning_simulator_amd.ops import ref
from distributed_learning_simulator_amd.parallel.comm import Comm
from distributed_learning_simulator_amd.session import Session
from distributed_learning_simulator_amd.utils import privacy
from distributed_learning_simulator_amd.worker import robust_worker as RW
from distributed_learning_simulator_amd.worker.aggregation_worker import AggregationWorker

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_distributed as TD  # noqa: E402  (the gloo launch helpers)

METRICS = ("dp_clipped_fraction", "dp_median_norm", "dp_rejected", "dp_epsilon", "dp_epsilon_poisson")


def _run(overrides, tmp_path, device="cpu", method="fed_dp_avg"):
    ov = {"round": 2, "epoch": 1, "worker_number": 5, "dataset_kwargs.scale": 0.04, **overrides}
    args = ["--config-name", f"{method}/mnist.yaml"] + [f"++{method}.{k}={v}" for k, v in ov.items()]
    args += [f"++{method}.save_dir={tmp_path}", f"++{method}.log_level=WARNING"]
    sess = Session(load_config(args), comm=Comm(device=torch.device(device)))
    return sess, sess.run()


def _bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _spy_rounds(monkeypatch, rounds):
    """Record per aggregation: θ_t, the accumulator after the noise, the fp64 result, the norms, the
    clipped and rejected client ids, the round's statistics."""
    orig = DA.DPFedAvgAlgorithm.aggregate_worker_data

    def agg_spy(self, old_parameter):
        old = old_parameter.detach().clone()
        rnd = self._round()
        msg = orig(self, old_parameter)
        rounds.append(dict(old=old, round=rnd, acc=self.last_acc.detach().clone(), new64=self.last_fp64.detach().clone(),
                           new=msg.parameter, norms=dict(self.last_norms), clipped_ids=list(self.last_clipped),
                           clipped=len(self.last_clipped), rejected=list(self.last_rejected), n=len(self.last_norms),
                           stats=dict(self.round_stats)))
        return msg

    monkeypatch.setattr(DA.DPFedAvgAlgorithm, "aggregate_worker_data", agg_spy)


def _spy_uploads(monkeypatch, uploads):
    """Record per upload wave: client ids, the honest rows, the rows actually uploaded (copies)."""
    base, byz = AggregationWorker._get_sent_data, RW.ByzantineWorker._get_sent_data
    honest = {}

    def base_spy(self, wave, theta_g, stats):
        msg = base(self, wave, theta_g, stats)
        honest["rows"] = msg.data.detach().clone()
        return msg

    def byz_spy(self, wave, theta_g, stats):
        msg = byz(self, wave, theta_g, stats)
        uploads.append((list(wave), honest["rows"], msg.data.detach().clone()))
        return msg

    monkeypatch.setattr(AggregationWorker, "_get_sent_data", base_spy)
    monkeypatch.setattr(RW.ByzantineWorker, "_get_sent_data", byz_spy)


def _uploads_by_round(uploads, rounds):
    """[[(client ids of the wave, honest rows, sent rows)]] per round: the waves in order, as many
    clients as the round aggregated."""
    out, it = [], iter(uploads)
    for r in rounds:
        waves, got = [], 0
        while got < r["n"]:
            wave, honest, sent = next(it)
            waves.append((wave, honest, sent))
            got += len(wave)
        out.append(waves)
    assert next(it, None) is None
    return out


def _oracle_acc(waves, clip):
    """The CPU oracle on a round's upload waves, in the order they were processed: (the clipped fp64
    sum, {client id: squared norm})."""
    acc, nsq_by_id = None, {}
    for wave, _, sent in waves:
        rows = sent.cpu()
        nsq = ref.row_sq_norms(rows)
        acc = ref.clipped_sum(rows, nsq, clip, out=acc)
        nsq_by_id.update(zip(wave, nsq.tolist()))
    return acc, nsq_by_id


def _oracle_round(r, waves, clip, z, m, seed, valid=None):
    """(the oracle's fp64 θ_{t+1} = θ_t + (clipped sum + z · C · noise) / m, the noise std on the mean).
    Also checks the session's norms, clipped and rejected ids against the oracle's."""
    acc, nsq = _oracle_acc(waves, clip)
    assert sorted(nsq) == sorted(r["norms"])
    for c, v in nsq.items():
        if math.isfinite(v):
            assert r["norms"][c] == math.sqrt(v)
        else:
            assert math.isnan(r["norms"][c]) and c in r["rejected"]
    assert r["rejected"] == sorted(c for c, v in nsq.items() if not math.isfinite(v))
    assert r["clipped_ids"] == sorted(c for c, v in nsq.items() if math.isfinite(v) and math.sqrt(v) > clip)
    if z > 0:
        ref.gaussian_add(acc, z * clip, seed, r["round"], valid)
    return r["old"].cpu().double() + acc / float(m), z * clip / m


# ------------------------------------------------------------------ registration and configs
def test_method_is_registered_and_configs_load():
    from distributed_learning_simulator_amd.algorithm.fed_avg_algorithm import FedAVGAlgorithm
    from distributed_learning_simulator_amd.method import CentralizedAlgorithmFactory
    from distributed_learning_simulator_amd.server.aggregation_server import AggregationServer
    from distributed_learning_simulator_amd.topology.endpoints import ClientEndpoint, ServerEndpoint

    reg = CentralizedAlgorithmFactory.config["fed_dp_avg"]
    assert reg["client_cls"] is RW.ByzantineWorker and reg["algorithm_cls"] is DA.DPFedAvgAlgorithm
    assert reg["server_cls"] is AggregationServer
    assert reg["client_endpoint_cls"] is ClientEndpoint and reg["server_endpoint_cls"] is ServerEndpoint
    assert issubclass(DA.DPFedAvgAlgorithm, FedAVGAlgorithm)
    for name in ("mnist", "cifar10"):
        cfg = load_config(["--config-name", f"fed_dp_avg/{name}.yaml"])
        assert cfg.distributed_algorithm == "fed_dp_avg"
        clip, z, delta = DA.dp_settings(cfg)
        assert clip > 0 and z > 0 and delta == 1e-5


# ------------------------------------------------------------------ CPU sessions
def test_round_is_the_oracle_clipped_sum_plus_noise_over_m(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy_rounds(monkeypatch, rounds)
    _spy_uploads(monkeypatch, uploads)
    clip, z = 0.025, 0.7
    sess, res = _run({"algorithm_kwargs.dp_clip_norm": clip, "algorithm_kwargs.dp_noise_multiplier": z}, tmp_path)
    assert res["performance"] and len(rounds) == 2 and [r["round"] for r in rounds] == [1, 2]
    valid = sess.layout.valid_mask()
    for r, waves in zip(rounds, _uploads_by_round(uploads, rounds)):
        assert r["n"] == 5 and r["clipped"] >= 1
        exp, _ = _oracle_round(r, waves, clip, z, 5, sess.config.seed, valid)
        assert torch.equal(_bits64(r["new64"]), _bits64(exp)) and torch.equal(r["new"], exp.float())
        assert (r["new64"] != r["old"].double())[valid].all()  # the noise reaches every parameter ...
        assert (_bits32(r["new"])[~valid] == 0).all()  # ... and no padding element: they stay +0
    assert torch.equal(sess.server.global_parameter, rounds[-1]["new"])


def test_noise_off_and_huge_clip_is_the_unweighted_mean(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy_rounds(monkeypatch, rounds)
    _spy_uploads(monkeypatch, uploads)
    ov = {"worker_number": 4, "algorithm_kwargs.dp_clip_norm": 1e30, "algorithm_kwargs.dp_noise_multiplier": 0}
    sess, _ = _run(ov, tmp_path / "dp")
    assert sess.worker.dataset_sizes([0, 1, 2, 3]).numel() == 4  # (dataset sizes exist and are ignored)
    for r, waves in zip(rounds, _uploads_by_round(uploads, rounds)):
        assert r["clipped"] == 0 and r["rejected"] == [] and r["stats"]["dp_epsilon"] == math.inf
        acc = torch.zeros(r["old"].numel(), dtype=torch.float64)
        for _, _, sent in waves:
            for row in sent:
                acc = acc + row.double()
        exp = r["old"].double() + acc / 4.0
        assert torch.equal(_bits64(r["new64"]), _bits64(exp))
    # ... which is what fed_multi_krum gives with nothing rejected (f = 0, m = n)
    mk = {"worker_number": 4, "algorithm_kwargs.byzantine_number": 0, "algorithm_kwargs.krum_f": 0,
          "algorithm_kwargs.krum_m": 4}
    other, _ = _run(mk, tmp_path / "mk", method="fed_multi_krum")
    assert torch.equal(_bits32(sess.server.global_parameter), _bits32(other.server.global_parameter))


def test_nan_attacker_is_rejected_and_counted_while_fed_avg_breaks(tmp_path, monkeypatch):
    rounds = []
    _spy_rounds(monkeypatch, rounds)
    attack = {"algorithm_kwargs.byzantine_number": 1, "algorithm_kwargs.byzantine_attack": "nan"}
    sess, _ = _run({**attack, "algorithm_kwargs.dp_clip_norm": 0.025}, tmp_path / "dp")
    assert torch.isfinite(sess.server.global_parameter).all()
    for r, row in zip(rounds, sess.metrics):
        assert r["rejected"] == [0] and math.isnan(r["norms"][0]) and row["dp_rejected"] == 1
    # the same upload in a plain weighted mean: ByzantineWorker under the FedAvg algorithm
    from distributed_learning_simulator_amd.algorithm.fed_avg_algorithm import FedAVGAlgorithm
    from distributed_learning_simulator_amd.method import CentralizedAlgorithmFactory

    reg = CentralizedAlgorithmFactory.config["fed_dp_avg"]
    monkeypatch.setitem(reg, "algorithm_cls", FedAVGAlgorithm)
    plain, _ = _run({**attack, "algorithm_kwargs.dp_clip_norm": 0.025}, tmp_path / "avg")
    assert type(plain.server.algorithm) is FedAVGAlgorithm
    assert not torch.isfinite(plain.server.global_parameter).all()


def test_sign_flip_attacker_moves_the_sum_by_at_most_the_clip_norm(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy_rounds(monkeypatch, rounds)
    _spy_uploads(monkeypatch, uploads)
    clip = 0.025
    ov = {"algorithm_kwargs.byzantine_number": 1, "algorithm_kwargs.byzantine_attack": "sign_flip",
          "algorithm_kwargs.byzantine_scale": 10, "algorithm_kwargs.dp_clip_norm": clip,
          "algorithm_kwargs.dp_noise_multiplier": 0}
    sess, _ = _run(ov, tmp_path)
    for r, waves in zip(rounds, _uploads_by_round(uploads, rounds)):
        rows = {c: (h[i], s[i]) for wave, h, s in waves for i, c in enumerate(wave)}
        honest, sent = rows[0]
        assert torch.equal(sent, honest * -10.0) and 0 in r["clipped_ids"]
        assert r["norms"][0] == pytest.approx(10.0 * float(honest.double().norm()), rel=1e-6) and r["norms"][0] > clip
        part = ref.clipped_sum(sent[None].cpu(), ref.row_sq_norms(sent[None].cpu()), clip)
        assert float(part.norm()) <= clip * (1.0 + 1e-12)
        # the sum without the attacker's clipped contribution is the others' clipped sum
        others, _ = _oracle_acc([([c], None, rows[c][1][None]) for c in sorted(rows) if c != 0], clip)
        moved = (r["acc"].cpu() - others).norm()
        assert float(moved) <= clip * (1.0 + 1e-9)


def test_client_failures_leave_the_denominator_at_m(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy_rounds(monkeypatch, rounds)
    _spy_uploads(monkeypatch, uploads)
    clip, z = 0.025, 0.5
    ov = {"round": 3, "worker_number": 8, "algorithm_kwargs.failure_rate": 0.4, "algorithm_kwargs.dp_clip_norm": clip,
          "algorithm_kwargs.dp_noise_multiplier": z}
    sess, _ = _run(ov, tmp_path)
    ns = [r["n"] for r in rounds]
    assert len(ns) == 3 and min(ns) < 8, ns
    assert sess.server.algorithm.denominator() == 8
    valid = sess.layout.valid_mask()
    for r, waves in zip(rounds, _uploads_by_round(uploads, rounds)):
        exp, _ = _oracle_round(r, waves, clip, z, 8, sess.config.seed, valid) if r["n"] else (None, None)
        if exp is not None:
            assert torch.equal(_bits64(r["new64"]), _bits64(exp))
    assert torch.isfinite(sess.server.global_parameter).all()


def test_random_client_number_is_the_denominator(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy_rounds(monkeypatch, rounds)
    _spy_uploads(monkeypatch, uploads)
    clip, z = 0.025, 0.5
    ov = {"worker_number": 8, "algorithm_kwargs.random_client_number": 3, "algorithm_kwargs.dp_clip_norm": clip,
          "algorithm_kwargs.dp_noise_multiplier": z}
    sess, _ = _run(ov, tmp_path)
    assert sess.server.algorithm.denominator() == 3
    valid = sess.layout.valid_mask()
    for r, waves, row in zip(rounds, _uploads_by_round(uploads, rounds), sess.metrics):
        assert r["n"] == 3
        exp, _ = _oracle_round(r, waves, clip, z, 3, sess.config.seed, valid)
        assert torch.equal(_bits64(r["new64"]), _bits64(exp))
        assert row["dp_epsilon_poisson"] == privacy.epsilon(z, r["round"], 1e-5, q=3 / 8) < row["dp_epsilon"]


def _algorithm(kwargs, P=48, worker_number=4, comm=None):
    alg = DA.DPFedAvgAlgorithm()
    alg.bind(types.SimpleNamespace(algorithm_kwargs=kwargs, debug=False, seed=7, worker_number=worker_number),
             types.SimpleNamespace(padded_size=P), "cpu", comm)
    return alg


def test_masked_packed_and_parameter_uploads_raise():
    theta = torch.zeros(48)
    alg = _algorithm({"dp_clip_norm": 1.0})
    with pytest.raises(RuntimeError, match="dense"):
        alg.process_worker_data(CohortMessage(client_ids=[0], dataset_sizes=torch.ones(1), kind="delta",
                                              data=torch.ones(1, 48), mask=torch.ones(1, 48, dtype=torch.bool)), theta)
    alg.clear_worker_data()
    with pytest.raises(RuntimeError, match="dense"):
        alg.process_worker_data(CohortMessage(client_ids=[0], dataset_sizes=torch.ones(1), kind="delta",
                                              data=torch.ones(1, 48), block_mask=torch.ones(1, 2, dtype=torch.bool)), theta)
    alg.clear_worker_data()
    with pytest.raises(RuntimeError, match="dense"):
        alg.process_worker_data(CohortMessage(client_ids=[0], dataset_sizes=torch.ones(1), kind="delta", data=None,
                                              payload=object()), theta)
    alg.clear_worker_data()
    with pytest.raises(RuntimeError, match="delta"):
        alg.process_worker_data(CohortMessage(client_ids=[0], dataset_sizes=torch.ones(1), kind="parameter",
                                              data=torch.ones(1, 48)), theta)
    alg.clear_worker_data()
    assert not alg.fuses_payload
    # dense deltas in two waves, dataset sizes ignored, the fixed denominator 4 for three uploads
    rows = torch.tensor([[3.0], [0.25], [-1.0]]).repeat(1, 48)
    alg = _algorithm({"dp_clip_norm": 2.0, "dp_noise_multiplier": 0})
    alg.process_worker_data(CohortMessage(client_ids=[2, 0], dataset_sizes=torch.tensor([100.0, 1.0]), kind="delta",
                                          data=rows[:2]), theta)
    alg.process_worker_data(CohortMessage(client_ids=[1], dataset_sizes=torch.ones(1), kind="delta", data=rows[2:]), theta)
    msg = alg.aggregate_worker_data(theta)
    n3 = math.sqrt(48 * 9.0)
    assert alg.last_norms == {0: math.sqrt(48 / 16.0), 1: math.sqrt(48.0), 2: n3}
    assert alg.last_clipped == [1, 2] and alg.last_rejected == []
    exp = (3.0 * (2.0 / n3) + 0.25) + -1.0 * (2.0 / math.sqrt(48.0))
    assert msg.parameter.tolist() == [float(torch.tensor(exp / 4.0, dtype=torch.float32))] * 48
    assert alg.round_stats["dp_clipped_fraction"] == 2 / 3 and alg.round_stats["dp_median_norm"] == math.sqrt(48.0)


@pytest.mark.parametrize("kwargs", [{}, {"dp_clip_norm": 0}, {"dp_clip_norm": -1.0}, {"dp_clip_norm": "nan"},
                                    {"dp_clip_norm": float("inf")}, {"dp_clip_norm": "abc"},
                                    {"dp_clip_norm": 1.0, "dp_noise_multiplier": -0.5},
                                    {"dp_clip_norm": 1.0, "dp_noise_multiplier": float("inf")},
                                    {"dp_clip_norm": 1.0, "dp_delta": 0}, {"dp_clip_norm": 1.0, "dp_delta": 1.0}])
def test_bad_kwargs_raise_at_construction(kwargs):
    with pytest.raises(ValueError, match="dp_"):
        _algorithm(kwargs)


def test_bad_kwargs_raise_when_the_session_is_built(tmp_path):
    args = ["--config-name", "fed_dp_avg/mnist.yaml", "++fed_dp_avg.algorithm_kwargs.dp_clip_norm=-2",
            f"++fed_dp_avg.save_dir={tmp_path}", "++fed_dp_avg.worker_number=2", "++fed_dp_avg.dataset_kwargs.scale=0.04"]
    with pytest.raises(ValueError, match="dp_clip_norm"):
        Session(load_config(args), comm=Comm(device=torch.device("cpu")))


def test_metrics_are_recorded_and_epsilon_grows(tmp_path):
    z = 0.9
    ov = {"round": 3, "algorithm_kwargs.dp_clip_norm": 0.025, "algorithm_kwargs.dp_noise_multiplier": z}
    sess, res = _run(ov, tmp_path)
    rows = sess.metrics
    assert [m["round"] for m in rows] == [1, 2, 3]
    for t, row in enumerate(rows, start=1):
        assert all(k in row for k in METRICS), sorted(row)
        assert 0.0 <= row["dp_clipped_fraction"] <= 1.0 and row["dp_median_norm"] > 0 and row["dp_rejected"] == 0
        assert row["dp_epsilon"] == privacy.epsilon(z, t, 1e-5)
        assert row["dp_epsilon_poisson"] == row["dp_epsilon"]  # every client every round: q = 1
    eps = [m["dp_epsilon"] for m in rows]
    assert eps[0] < eps[1] < eps[2] < math.inf
    # ... and for this method only
    other, _ = _run({"round": 1}, tmp_path / "avg", method="fed_avg")
    assert not any(k in other.metrics[0] for k in METRICS)


def test_checkpoint_resume_reproduces_run(tmp_path):
    base = {"round": 3, "worker_number": 5, "checkpoint_every": 1, "algorithm_kwargs.dp_clip_norm": 0.025,
            "algorithm_kwargs.byzantine_number": 1}
    full, res_full = _run(base, tmp_path / "full")
    assert (tmp_path / "full" / "checkpoint.pt").exists()
    _run({**base, "round": 2}, tmp_path / "part")
    resumed, res = _run({**base, "resume_from": str(tmp_path / "part" / "checkpoint.pt")}, tmp_path / "resumed")
    torch.testing.assert_close(resumed.server.global_parameter, full.server.global_parameter, rtol=0, atol=0)
    assert sorted(res["performance"]) == sorted(res_full["performance"])
    assert [m["round"] for m in resumed.metrics] == [1, 2, 3]
    assert resumed.metrics[-1]["dp_epsilon"] == full.metrics[-1]["dp_epsilon"]


# ------------------------------------------------------------------ ranks
DP = {"algorithm_kwargs": {"dp_clip_norm": 0.05, "dp_noise_multiplier": 0.6}}


def test_two_gloo_ranks_match_single_rank(tmp_path):
    """World 2 against 1 rank within the tolerance of the FedAvg gloo test (tests/test_distributed.py:
    rtol 1e-4, atol 1e-5 — the fp64 partial sums of the ranks are added in another order, and fp32
    client deltas may differ in the last bit between cohort compositions); replicas identical."""
    theta1, res1 = TD._single("fed_dp_avg", str(tmp_path / "s"), DP)
    outs = TD._run_world(2, "fed_dp_avg", str(tmp_path / "d"), DP)
    th0 = outs[0][1]
    for o in outs[1:]:
        torch.testing.assert_close(o[1], th0, rtol=0, atol=0)
    print("max |theta(world 2) - theta(1 rank)|:", float((th0 - theta1).abs().max()))
    torch.testing.assert_close(th0, theta1, rtol=1e-4, atol=1e-5)
    assert outs[0][3] == res1["bytes_up"]


def _client_row(c: int, P: int) -> torch.Tensor:
    if c == 4:
        return torch.full((P,), float("nan"))
    return torch.randn(P, generator=torch.Generator().manual_seed(77 + c)) * (50.0 if c == 1 else 1.0)


def _nn(out):
    """(norms with NaN as None, clipped ids, rejected ids) of one `_aggregate` round: comparable with ==."""
    return {c: None if v != v else v for c, v in out[2].items()}, out[3], out[4]


def _aggregate(cohorts, comm, z, P=2 * ref.PAIR_SPAN + 48):
    """Feed fixed uploads (rows keyed by client id) to the algorithm on this rank and aggregate twice
    (two rounds: two noise streams)."""
    alg = _algorithm({"dp_clip_norm": 200.0, "dp_noise_multiplier": z}, P=P, worker_number=7, comm=comm)
    theta = torch.linspace(-1.0, 1.0, P)
    out = []
    for _ in range(2):
        for ids in cohorts:
            rows = torch.stack([_client_row(c, P) for c in ids])
            alg.process_worker_data(CohortMessage(client_ids=list(ids), dataset_sizes=torch.ones(len(ids)),
                                                  kind="delta", data=rows), theta)
        msg = alg.aggregate_worker_data(theta)
        out.append((msg.parameter.numpy().copy(), alg.last_acc.numpy().copy(), dict(alg.last_norms),
                    list(alg.last_clipped), list(alg.last_rejected)))
        alg.clear_worker_data()
        theta = msg.parameter
    return out


def _agg_worker(rank, world, port, shards, z, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DLS_FORCE_CPU="1")
    torch.set_num_threads(1)
    from distributed_learning_simulator_amd.parallel import comm as commmod

    commmod._COMM = None
    c = commmod.init_distributed(prefer_gpu=False)
    q.put((rank, _aggregate(shards[rank], c, z)))
    commmod.shutdown()


def test_noise_on_two_gloo_ranks_is_bitwise_the_single_rank_noise():
    """The same uploads on one rank and spread over two (one of them in two waves, a NaN upload): the
    noise every rank adds is the single rank's bit for bit — isolated as the accumulator with noise
    minus the accumulator without, which is exact where the clipped sums agree — and the norms, the
    clipped and the rejected clients are the same."""
    import torch.multiprocessing as mp

    shards = [[[0, 1], [2]], [[6, 5, 4, 3]]]
    everyone = sorted(c for rank in shards for wave in rank for c in wave)
    single = {z: _aggregate([everyone], Comm(), z) for z in (0.0, 1.5)}
    ctx = mp.get_context("spawn")
    results = {}
    for z in (0.0, 1.5):
        q = ctx.Queue()
        port = TD._free_port()
        procs = [ctx.Process(target=_agg_worker, args=(r, 2, port, shards, z, q)) for r in range(2)]
        for p in procs:
            p.start()
        outs = dict(q.get(timeout=300) for _ in procs)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        results[z] = outs
    P = 2 * ref.PAIR_SPAN + 48
    for rnd in range(2):
        s0, s1 = single[0.0][rnd], single[1.5][rnd]
        assert _nn(s1) == _nn(s0) and s1[3] == [1] and s1[4] == [4]  # the far upload clipped, the NaN one rejected
        oracle = ref.gaussian_noise(P, 7, rnd + 1) * (1.5 * 200.0)
        for rank in range(2):
            w0, w1 = results[0.0][rank][rnd], results[1.5][rank][rnd]
            assert _nn(w1) == _nn(s1) == _nn(w0)
            # both ranks hold the same accumulator, and the same θ
            assert torch.equal(_bits64(torch.from_numpy(w1[1])), _bits64(torch.from_numpy(results[1.5][0][rnd][1])))
            assert torch.equal(_bits32(torch.from_numpy(w1[0])), _bits32(torch.from_numpy(results[1.5][0][rnd][0])))
            torch.testing.assert_close(torch.from_numpy(w1[0]), torch.from_numpy(s1[0]), rtol=1e-4, atol=1e-5)
        # the noise itself: added to an accumulator, it is fl(acc + t); recover t where that is exact
        for noisy, plain in ((s1[1], s0[1]), (results[1.5][0][rnd][1], results[0.0][0][rnd][1]),
                             (results[1.5][1][rnd][1], results[0.0][1][rnd][1])):
            plain_t = torch.from_numpy(plain)
            want = plain_t + oracle  # the oracle's noise added to this accumulator: the same single rounding
            assert torch.equal(_bits64(torch.from_numpy(noisy)), _bits64(want))
