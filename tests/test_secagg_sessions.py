"""fed_secagg sessions: secure aggregation as a registered method (method/fed_secagg, worker/secagg_worker,
algorithm/secagg_algorithm, utils/secagg_protocol). Every comparison with the oracle is bit for bit."""

import os
import sys
import types

import pytest
import torch

from distributed_learning_simulator_amd.algorithm import secagg_algorithm as SA
from distributed_learning_simulator_amd.config import load_config
from distributed_learning_simulator_amd.message import CohortMessage
from distributed_learning_simulator_amd.ops import compress, fl, ref
from distributed_learning_simulator_amd.parallel.comm import Comm
from distributed_learning_simulator_amd.session import Session
from distributed_learning_simulator_amd.utils import secagg_protocol as SP
from distributed_learning_simulator_amd.worker import secagg_worker as SW
from distributed_learning_simulator_amd.worker.aggregation_worker import AggregationWorker

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_distributed as TD  # noqa: E402  (the gloo launch helpers)

METRICS = ("secagg_survivors", "secagg_dropped", "secagg_aborted", "secagg_clamped_fraction", "secagg_nan_elements",
           "secagg_frac_bits", "secagg_mask_streams", "secagg_dropped_bytes")


def _run(overrides, tmp_path, device="cpu", method="fed_secagg"):
    ov = {"round": 2, "epoch": 1, "worker_number": 5, "dataset_kwargs.scale": 0.04, "algorithm_kwargs.failure_rate": 0,
          **overrides}
    args = ["--config-name", f"{method}/mnist.yaml"] + [f"++{method}.{k}={v}" for k, v in ov.items()]
    args += [f"++{method}.save_dir={tmp_path}", f"++{method}.log_level=ERROR"]
    sess = Session(load_config(args), comm=Comm(device=torch.device(device)))
    return sess, sess.run()


def _bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _spy(monkeypatch, rounds, uploads):
    """Per upload wave: (round, selected ids, wave ids, the delta rows before masking, the payload rows, the
    counters, the wire bytes) as copies; per aggregation: θ_t, the fp64 result, the new θ, the statistics."""
    base, masked = AggregationWorker._get_sent_data, SW.SecAggWorker._get_sent_data
    clear = {}

    def base_spy(self, wave, theta_g, stats):
        msg = base(self, wave, theta_g, stats)
        clear["rows"] = msg.data.detach().clone()
        return msg

    def masked_spy(self, wave, theta_g, stats):
        msg = masked(self, wave, theta_g, stats)
        uploads.append(dict(round=self._round_num, selected=self._selected(), wave=list(wave), clear=clear["rows"].cpu(),
                            words=msg.payload.rows.detach().clone().cpu(), counters=msg.extra["secagg_stats"].cpu(),
                            wire=list(msg.payload.row_bytes())))
        return msg

    orig = SA.SecAggAlgorithm.aggregate_worker_data

    def agg_spy(self, old_parameter):
        old, rnd = old_parameter.detach().clone().cpu(), self._round()
        msg = orig(self, old_parameter)
        rounds.append(dict(old=old, round=rnd, new64=self.last_fp64.detach().clone().cpu(), new=msg.parameter.cpu(),
                           reporting=list(self.last_reporting), dropped=list(self.last_dropped),
                           stats=dict(self.round_stats)))
        return msg

    monkeypatch.setattr(AggregationWorker, "_get_sent_data", base_spy)
    monkeypatch.setattr(SW.SecAggWorker, "_get_sent_data", masked_spy)
    monkeypatch.setattr(SA.SecAggAlgorithm, "aggregate_worker_data", agg_spy)


def _oracle_round(r, waves, seed, R, f, degree=0, threshold=None):
    """The oracle on one round's spied uploads: checks every payload row against `ref.secagg_mask_rows` with an
    entry table built here, and returns fp64(θ_t) + (Σ_S q) · 2^−f / |S| (θ_t itself if nobody reported)."""
    qsum, ids = None, []
    for up in waves:
        assert up["round"] == r["round"]
        proto = SP.RoundProtocol(seed, up["round"], up["selected"], degree, threshold)  # (not the cached one)
        offsets, keys, signs = proto.entry_table(up["wave"])
        want, counters = ref.secagg_mask_rows(up["clear"], offsets, keys, signs, R, f)
        assert torch.equal(up["words"], want) and torch.equal(up["counters"], counters)
        assert offsets[-1] == sum(proto.degree_of(c) + 1 for c in up["wave"])
        q, _ = ref.secagg_quantise(up["clear"], R, f)
        qsum = q.sum(0) if qsum is None else qsum + q.sum(0)
        ids += up["wave"]
    assert sorted(ids) == r["reporting"]
    if not ids:
        return r["old"].double()
    return r["old"].double() + (qsum.double() * 2.0 ** -f) / float(len(ids))


def _by_round(uploads, rounds):
    return [[u for u in uploads if u["round"] == r["round"]] for r in rounds]


# ------------------------------------------------------------------ registration and configs
def test_method_is_registered_and_configs_load():
    from distributed_learning_simulator_amd.algorithm.fed_avg_algorithm import FedAVGAlgorithm
    from distributed_learning_simulator_amd.method import CentralizedAlgorithmFactory
    from distributed_learning_simulator_amd.server.aggregation_server import AggregationServer
    from distributed_learning_simulator_amd.topology.endpoints import ClientEndpoint, ServerEndpoint

    reg = CentralizedAlgorithmFactory.config["fed_secagg"]
    assert reg["client_cls"] is SW.SecAggWorker and reg["algorithm_cls"] is SA.SecAggAlgorithm
    assert reg["server_cls"] is AggregationServer
    assert reg["client_endpoint_cls"] is ClientEndpoint and reg["server_endpoint_cls"] is ServerEndpoint
    assert issubclass(SA.SecAggAlgorithm, FedAVGAlgorithm) and issubclass(SW.SecAggWorker, AggregationWorker)
    cfg = load_config(["--config-name", "fed_secagg/mnist.yaml"])
    assert SA.secagg_settings(cfg) == (0.5, 28, 0, None)  # 10 · 0.5 · 2^28 ≤ 2^31 − 1 < 10 · 0.5 · 2^29
    cfg = load_config(["--config-name", "fed_secagg/cifar10.yaml"])
    assert SA.secagg_settings(cfg) == (1.0, 26, 8, 5) and SA.cohort_size(cfg) == 20


# ------------------------------------------------------------------ CPU sessions
def test_round_is_the_oracle_sum_of_the_quantised_deltas(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy(monkeypatch, rounds, uploads)
    sess, res = _run({"algorithm_kwargs.secagg_range": 0.05}, tmp_path)
    R, f = fl.secagg_frac_bits(0.05, 5)
    alg = sess.server.algorithm
    assert (alg.range, alg.frac_bits) == (R, f) and res["performance"] and [r["round"] for r in rounds] == [1, 2]
    valid = sess.layout.valid_mask()
    dense = 4 * sess.layout.num_params
    for r, waves, row in zip(rounds, _by_round(uploads, rounds), sess.metrics):
        exp = _oracle_round(r, waves, sess.config.seed, R, f)
        assert torch.equal(_bits64(r["new64"]), _bits64(exp)) and torch.equal(r["new"], exp.float())
        assert r["reporting"] == [0, 1, 2, 3, 4] and r["dropped"] == []
        assert (r["new"][~valid].view(torch.int32) == 0).all()  # the padding cancels to exactly 0
        assert all(k in row for k in METRICS)
        assert row["secagg_survivors"] == 5 and row["secagg_dropped"] == row["secagg_aborted"] == 0
        assert row["secagg_frac_bits"] == f and row["secagg_mask_streams"] == 5 * 5 + 5 and row["secagg_dropped_bytes"] == 0
        assert row["secagg_nan_elements"] == 0 and 0.0 <= row["secagg_clamped_fraction"] < 1.0
        wire = [b for u in waves for b in u["wire"]]
        assert wire == [dense + 16 + 48 * 4] * 5 and row["comm_bytes_up"] == sum(wire)
        # the masked words say nothing about the clear code
        for u in waves:
            q, _ = ref.secagg_quantise(u["clear"], R, f)
            assert ((u["words"].long() != q).double().mean(1) > 0.99).all()
    assert res["bytes_up"] == 2 * 5 * (dense + 16 + 48 * 4)
    assert torch.equal(sess.server.global_parameter, rounds[-1]["new"])
    other, _ = _run({"round": 1}, tmp_path / "avg", method="fed_avg")
    assert not any(k in other.metrics[0] for k in METRICS)


def test_dropouts_are_recovered_on_the_survivors(tmp_path, monkeypatch):
    """failure_rate 0.3 with the configs' default seed 0 drops client 6 in round 1, client 2 in round 2 and clients
    3 and 7 in round 3 of 8 (found by running it); the complete graph with t = 4 of 7 recovers all of them."""
    rounds, uploads = [], []
    _spy(monkeypatch, rounds, uploads)
    ov = {"round": 3, "worker_number": 8, "algorithm_kwargs.failure_rate": 0.3, "algorithm_kwargs.secagg_range": 0.05}
    sess, _ = _run(ov, tmp_path)
    R, f = fl.secagg_frac_bits(0.05, 8)
    dropped = [r["dropped"] for r in rounds]
    print("dropped per round:", dropped)
    assert dropped == [[6], [2], [3, 7]] and not any(r["stats"]["secagg_aborted"] for r in rounds)
    for r, waves in zip(rounds, _by_round(uploads, rounds)):
        n, nd = len(r["reporting"]), len(r["dropped"])
        assert n + nd == 8 and r["stats"]["secagg_survivors"] == n and r["stats"]["secagg_dropped"] == nd
        exp = _oracle_round(r, waves, sess.config.seed, R, f)
        assert torch.equal(_bits64(r["new64"]), _bits64(exp))
        assert r["stats"]["secagg_mask_streams"] == n * 8 + n + nd * n
        assert r["stats"]["secagg_dropped_bytes"] == nd * (16 + 32 * 7)
    # the dropped clients' key and share bytes are not part of the uplink count
    assert [m["comm_bytes_up"] for m in sess.metrics] == [len(r["reporting"]) * (4 * sess.layout.num_params + 16 + 48 * 7)
                                                          for r in rounds]


def test_abort_leaves_the_model_unchanged(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy(monkeypatch, rounds, uploads)
    # t = d: any dropout aborts. Seed 0 at failure_rate 0.3 drops nobody of 6 in round 1, client 2 in round 2 and
    # client 3 in round 3 (found by running it)
    ov = {"round": 3, "worker_number": 6, "algorithm_kwargs.failure_rate": 0.3, "algorithm_kwargs.secagg_range": 0.05,
          "algorithm_kwargs.secagg_degree": 2, "algorithm_kwargs.secagg_threshold": 2}
    sess, _ = _run(ov, tmp_path)
    assert [r["dropped"] for r in rounds] == [[], [2], [3]]
    assert [r["stats"]["secagg_aborted"] for r in rounds] == [0, 1, 1]
    for r, row in zip(rounds, sess.metrics):
        assert row["secagg_aborted"] == r["stats"]["secagg_aborted"] == (1 if r["dropped"] else 0)
        if r["dropped"]:
            assert torch.equal(_bits64(r["new64"]), _bits64(r["old"].double())) and torch.equal(r["new"], r["old"])
        else:
            assert not torch.equal(r["new"], r["old"])


def test_generous_range_is_the_unweighted_mean_to_half_a_unit(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy(monkeypatch, rounds, uploads)
    sess, _ = _run({"algorithm_kwargs.secagg_range": 4.0}, tmp_path)
    R, f = fl.secagg_frac_bits(4.0, 5)
    valid = sess.layout.valid_mask()
    for r, waves in zip(rounds, _by_round(uploads, rounds)):
        assert r["stats"]["secagg_clamped_fraction"] == 0.0
        deltas = torch.cat([u["clear"] for u in waves]).double()
        assert deltas.shape[0] == 5 and float(deltas.abs().max()) < R
        mean = r["old"].double() + deltas.sum(0) / 5.0
        # each q is within half a unit of the scaled delta, the mean of 5 such errors is no larger; one ulp
        # of fp64 at the magnitudes involved for the additions on both sides
        bound = 2.0 ** -(f + 1) + 2.0 ** -52 * (r["old"].double().abs() + deltas.abs().sum(0))
        err = (r["new64"] - mean).abs()
        print("max err in units of 2^-(f+1):", float(err.max()) * 2.0 ** (f + 1))
        assert (err <= bound).all() and (err[valid] > 0).any()


def test_bad_settings_raise_when_the_session_is_built(tmp_path):
    def build(**kw):
        args = ["--config-name", "fed_secagg/mnist.yaml", f"++fed_secagg.save_dir={tmp_path}", "++fed_secagg.worker_number=4",
                "++fed_secagg.dataset_kwargs.scale=0.04"] + [f"++fed_secagg.{k}={v}" for k, v in kw.items()]
        return Session(load_config(args), comm=Comm(device=torch.device("cpu")))

    for bad in ("null", 0, -1.0, "inf", "nan"):
        with pytest.raises(ValueError, match="secagg"):
            build(**{"algorithm_kwargs.secagg_range": bad})
    with pytest.raises(ValueError, match="overflows the ring"):
        build(**{"algorithm_kwargs.secagg_frac_bits": 30})
    with pytest.raises(ValueError, match="even"):
        build(**{"worker_number": 8, "algorithm_kwargs.secagg_degree": 3})
    for t in (0, 4):
        with pytest.raises(ValueError, match="secagg_threshold"):
            build(**{"algorithm_kwargs.secagg_threshold": t})
    with pytest.raises(RuntimeError, match="deltas"):
        build(distribute_init_parameters=False)


def _algorithm(kwargs, P=48, worker_number=4, comm=None, selected=None, rnd=1):
    alg = SA.SecAggAlgorithm()
    server = types.SimpleNamespace(round_number=rnd, selected=list(range(worker_number) if selected is None else selected))
    alg.bind(types.SimpleNamespace(algorithm_kwargs=kwargs, debug=False, seed=7, worker_number=worker_number),
             types.SimpleNamespace(padded_size=P, num_params=P - 7), "cpu", comm, server)
    return alg


def _message(alg, ids, rows):
    proto = SP.round_protocol(7, alg.server.round_number, alg.server.selected, alg.degree, alg.threshold)
    words, counters = fl.secagg_mask_rows(rows, proto.entry_table(ids), alg.range, alg.frac_bits)
    return CohortMessage(client_ids=list(ids), dataset_sizes=torch.ones(len(ids)), kind="delta", data=None,
                         payload=compress.MaskedPayload(words, [proto.row_bytes(c, 41) for c in ids]),
                         extra={"secagg_stats": counters})


def test_foreign_uploads_raise():
    theta = torch.zeros(48)
    alg = _algorithm({"secagg_range": 1.0})
    ok = _message(alg, [0], torch.ones(1, 48))
    for change, match in ((dict(mask=torch.ones(1, 48, dtype=torch.bool)), "masks"),
                          (dict(block_mask=torch.ones(1, 2, dtype=torch.bool)), "masks"),
                          (dict(kind="parameter"), "delta"), (dict(payload=None, data=torch.ones(1, 48)), "MaskedPayload"),
                          (dict(payload=compress.SparsePayload(None, None, None, 1)), "MaskedPayload")):
        msg = CohortMessage(**{**{f: getattr(ok, f) for f in ("client_ids", "dataset_sizes", "kind", "data", "payload",
                                                             "extra")}, **change})
        with pytest.raises(RuntimeError, match=match):
            alg.process_worker_data(msg, theta)
        alg.clear_worker_data()
    assert alg.fuses_payload
    with pytest.raises(RuntimeError, match="no dense form"):
        ok.payload.decode()
    with pytest.raises(RuntimeError, match="no dense form"):
        ok.dense()
    from distributed_learning_simulator_amd.topology.endpoints import StochasticQuantClientEndpoint

    cfg = load_config(["--config-name", "fed_secagg/mnist.yaml"])
    with pytest.raises(RuntimeError, match="quantising"):
        SW.SecAggWorker(cfg, StochasticQuantClientEndpoint())


def test_nobody_reported_leaves_the_model_unchanged():
    theta = torch.linspace(-1, 1, 48)
    alg = _algorithm({"secagg_range": 1.0})
    msg = alg.aggregate_worker_data(theta)
    assert torch.equal(msg.parameter, theta) and alg.round_stats["secagg_survivors"] == 0
    assert alg.round_stats["secagg_dropped"] == 4 and alg.round_stats["secagg_aborted"] == 0


def test_checkpoint_resume_reproduces_run(tmp_path):
    base = {"round": 3, "worker_number": 6, "checkpoint_every": 1, "algorithm_kwargs.secagg_range": 0.05,
            "algorithm_kwargs.failure_rate": 0.3, "algorithm_kwargs.secagg_degree": 4, "algorithm_kwargs.secagg_threshold": 1}
    full, res_full = _run(base, tmp_path / "full")
    assert (tmp_path / "full" / "checkpoint.pt").exists()
    _run({**base, "round": 2}, tmp_path / "part")
    resumed, res = _run({**base, "resume_from": str(tmp_path / "part" / "checkpoint.pt")}, tmp_path / "resumed")
    assert torch.equal(resumed.server.global_parameter.view(torch.int32), full.server.global_parameter.view(torch.int32))
    assert [m["round"] for m in resumed.metrics] == [1, 2, 3]
    for k in METRICS:
        assert resumed.metrics[-1][k] == full.metrics[-1][k]
    assert any(m["secagg_dropped"] for m in full.metrics)


def test_server_optimizer_steps_behind_it(tmp_path, monkeypatch):
    rounds, uploads = [], []
    _spy(monkeypatch, rounds, uploads)
    ov = {"algorithm_kwargs.secagg_range": 0.05, "algorithm_kwargs.server_optimizer": "adam",
          "algorithm_kwargs.server_lr": 0.02}
    sess, _ = _run(ov, tmp_path)
    R, f = fl.secagg_frac_bits(0.05, 5)
    P = rounds[0]["old"].numel()
    tau = 1e-3
    theta, m, v = rounds[0]["old"].clone(), torch.zeros(P, dtype=torch.float64), torch.full((P,), tau * tau,
                                                                                             dtype=torch.float64)
    for r, waves in zip(rounds, _by_round(uploads, rounds)):
        assert torch.equal(r["old"], theta)
        target = _oracle_round(r, waves, sess.config.seed, R, f)
        assert torch.equal(_bits64(r["new64"]), _bits64(target))
        ref.server_opt_step(theta, target, m, v, "adam", 0.02, 0.9, 0.99, tau, 1.0 - 0.9, 1.0 - 0.99)
    assert torch.equal(sess.server.global_parameter.view(torch.int32), theta.view(torch.int32))
    assert torch.equal(_bits64(sess.server.server_optimizer.m), _bits64(m))


# ------------------------------------------------------------------ ranks
def _client_row(c: int, P: int) -> torch.Tensor:
    row = torch.randn(P, generator=torch.Generator().manual_seed(31 + c)) * (3.0 if c == 1 else 0.2)
    row[41:] = 0
    if c == 5:
        row[3] = float("nan")
    return row


SELECTED = [0, 1, 2, 3, 4, 5, 6]
KW = {"secagg_range": 1.0, "secagg_degree": 4, "secagg_threshold": 2}


def _aggregate(cohorts, comm, P=48):
    """Feed fixed uploads (rows keyed by client id) to the algorithm on this rank and aggregate two rounds."""
    theta = torch.linspace(-1.0, 1.0, P)
    out = []
    for rnd in (1, 2):
        alg = _algorithm(KW, P=P, worker_number=7, comm=comm, selected=SELECTED, rnd=rnd)
        for ids in cohorts:
            if ids:
                alg.process_worker_data(_message(alg, ids, torch.stack([_client_row(c, P) for c in ids])), theta)
        msg = alg.aggregate_worker_data(theta)
        out.append((msg.parameter.numpy().copy(), alg.last_fp64.numpy().copy(), list(alg.last_reporting),
                    list(alg.last_dropped), dict(alg.round_stats)))
        theta = msg.parameter
    return out


def _agg_worker(rank, world, port, shards, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), DLS_FORCE_CPU="1")
    torch.set_num_threads(1)
    from distributed_learning_simulator_amd.parallel import comm as commmod

    commmod._COMM = None
    c = commmod.init_distributed(prefer_gpu=False)
    q.put((rank, _aggregate(shards[rank], c)))
    commmod.shutdown()


def test_two_gloo_ranks_are_bitwise_the_single_rank():
    """The same uploads on one rank and spread over two (one of them in two waves). Client 3 dropped: on the degree-4
    ring its partners 1, 2 live on rank 0 and 4, 5 on rank 1, so each rank's partial sum holds masks that only
    the other rank's rows and the recovery remove."""
    import torch.multiprocessing as mp

    shards = [[[0, 1], [2]], [[6, 5, 4]]]
    everyone = sorted(c for rank in shards for wave in rank for c in wave)
    single = _aggregate([everyone], Comm())
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = TD._free_port()
    procs = [ctx.Process(target=_agg_worker, args=(r, 2, port, shards, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    R, f = fl.secagg_frac_bits(1.0, 7)
    theta = torch.linspace(-1.0, 1.0, 48)
    for rnd in range(2):
        s = single[rnd]
        assert s[2] == everyone and s[3] == [3] and s[4]["secagg_aborted"] == 0 and s[4]["secagg_nan_elements"] == 1
        q_sum = ref.secagg_quantise(torch.stack([_client_row(c, 48) for c in everyone]), R, f)[0].sum(0)
        want = theta.double() + q_sum.double() * 2.0 ** -f / 6.0
        assert torch.equal(_bits64(torch.from_numpy(s[1])), _bits64(want))
        for rank in range(2):
            w = outs[rank][rnd]
            assert torch.equal(_bits64(torch.from_numpy(w[1])), _bits64(want)) and w[2:] == s[2:]
            assert torch.equal(torch.from_numpy(w[0]), torch.from_numpy(s[0]))
        theta = torch.from_numpy(s[0])
