"""fed_drive sessions: 1-bit rotated uploads as a registered method (method/fed_drive,
worker/error_feedback_worker.RotSignWorker, ops/compress.RotSignPayload), without and with error feedback."""

import os
import sys

import pytest
import torch

from distributed_learning_simulator_amd.config import load_config
from distributed_learning_simulator_amd.ops import compress, fl
from distributed_learning_simulator_amd.parallel.comm import Comm
from distributed_learning_simulator_amd.session import Session

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_distributed as TD  # noqa: E402  (the gloo launch helpers)

CFG = "fed_drive/mnist.yaml"
SMALL = {"epoch": 1, "worker_number": 3, "dataset_kwargs.scale": 0.04}


def _run(overrides, tmp_path, device="cpu"):
    args = ["--config-name", CFG] + [f"++fed_drive.{k}={v}" for k, v in overrides.items()]
    args += [f"++fed_drive.save_dir={tmp_path}", "++fed_drive.log_level=WARNING"]
    sess = Session(load_config(args), comm=Comm(device=torch.device(device)))
    return sess, sess.run()


def _nb(sess) -> int:
    return -(-sess.layout.padded_size // 4096)


def _spy(monkeypatch, name, calls):
    """Record the arguments (copies), the payload and the residual after of every call of compress.<name>."""
    orig = getattr(compress, name)

    def spy(delta, *rest, **kw):
        before = [a.detach().clone() if torch.is_tensor(a) else a for a in (delta, *rest)]
        p = orig(delta, *rest, **kw)
        after = rest[0].detach().clone() if torch.is_tensor(rest[0]) else None
        calls.append((before, kw, p, after))
        return p

    monkeypatch.setattr(compress, name, spy)


def test_fed_drive_is_registered_with_the_rotsign_worker():
    from distributed_learning_simulator_amd.method import CentralizedAlgorithmFactory
    from distributed_learning_simulator_amd.worker.error_feedback_worker import ErrorFeedbackWorker, RotSignWorker

    reg = CentralizedAlgorithmFactory.config["fed_drive"]
    assert reg["client_cls"] is RotSignWorker and issubclass(RotSignWorker, ErrorFeedbackWorker)


def test_fed_drive_unbiased_runs_without_client_state(tmp_path, monkeypatch):
    calls = []
    _spy(monkeypatch, "pack_rotsign", calls)
    rounds, workers = 2, 3
    sess, res = _run({**SMALL, "round": rounds}, tmp_path)
    assert res["bytes_up"] == rounds * workers * _nb(sess) * 516
    assert res["performance"]
    for stat in res["performance"].values():
        assert 0.0 <= stat["test_accuracy"] <= 1.0
    assert sess.worker.error_feedback is False and sess.worker._error is None
    assert sess.worker.state_dict() == {}
    assert len(calls) == rounds and all(c[1] == {"scale": "unbiased"} for c in calls)
    # the diagonal is keyed by (round's upload seed, client id): new every round
    seeds = [c[0][2] for c in calls]
    assert seeds[0] == fl.row_seeds(sess.worker.upload_seed(1), [0, 1, 2])
    assert seeds[1] == fl.row_seeds(sess.worker.upload_seed(2), [0, 1, 2]) and seeds[0] != seeds[1]


def test_fed_drive_unbiased_partial_participation(tmp_path):
    rounds = 3
    sess, res = _run({**SMALL, "round": rounds, "worker_number": 4, "algorithm_kwargs.random_client_number": 2},
                     tmp_path)
    assert res["bytes_up"] == rounds * 2 * _nb(sess) * 516
    assert sess.worker._error is None and torch.isfinite(sess.server.global_parameter).all()


def test_fed_drive_error_feedback_keeps_the_residual(tmp_path, monkeypatch):
    calls = []
    _spy(monkeypatch, "pack_rotsign_ef", calls)
    rounds, workers = 2, 3
    sess, res = _run({**SMALL, "round": rounds, "algorithm_kwargs.error_feedback": True}, tmp_path)
    assert res["bytes_up"] == rounds * workers * _nb(sess) * 516
    assert len(calls) == rounds
    # round 2 starts from round 1's residual, and the worker's residual is u − decode(payload) of round 2
    ((_, e1_before, _, _), _, _, e1_after), ((d2, e2_before, _, _), _, p2, e2_after) = calls
    assert e1_before.abs().sum() == 0
    assert torch.equal(e2_before, e1_after) and e2_before.abs().sum() > 0
    valid = sess.layout.valid_mask()
    exp = torch.where(valid, (d2 + e2_before) - p2.decode(), torch.zeros(()))
    assert exp.abs().sum() > 0
    assert torch.equal(sess.worker._error, exp) and torch.equal(e2_after, exp)
    assert torch.equal(sess.worker.state_dict()["error"], exp)


@pytest.mark.parametrize("ef", [False, True])
def test_fed_drive_checkpoint_resume_reproduces_run(tmp_path, ef):
    base = {**SMALL, "round": 3, "checkpoint_every": 1, "algorithm_kwargs.error_feedback": ef}
    full, res_full = _run(base, tmp_path / "full")
    assert (tmp_path / "full" / "checkpoint.pt").exists()
    part, _ = _run({**base, "round": 2}, tmp_path / "part")
    resumed, res = _run({**base, "resume_from": str(tmp_path / "part" / "checkpoint.pt")}, tmp_path / "resumed")
    assert torch.equal(resumed.server.global_parameter, full.server.global_parameter)
    if ef:
        assert part.worker._error.abs().sum() > 0
        assert torch.equal(resumed.worker._error, full.worker._error)
    else:
        assert resumed.worker._error is None and full.worker._error is None
    assert sorted(res["performance"]) == sorted(res_full["performance"])
    assert [m["round"] for m in resumed.metrics] == [1, 2, 3]


@pytest.mark.parametrize("ef", [False, True])
def test_fed_drive_two_ranks_equal_single_rank_bitwise(tmp_path, ef):
    extra = {"algorithm_kwargs": {"error_feedback": ef}}
    theta1, res1 = TD._single("fed_drive", str(tmp_path / "s"), extra)
    outs = TD._run_world(2, "fed_drive", str(tmp_path / "d"), extra)
    for o in outs:
        assert torch.equal(o[1], theta1)
    assert outs[0][3] == res1["bytes_up"]
    for key in res1["performance"]:
        assert outs[0][2][key]["test_accuracy"] == res1["performance"][key]["test_accuracy"]


# ------------------------------------------------------------------ GPU sessions
@pytest.mark.gpu
@pytest.mark.parametrize("ef", [False, True])
def test_fed_drive_gpu_sessions_are_reproducible(hip, tmp_path, ef):
    ov = {"round": 2, "epoch": 1, "worker_number": 4, "dataset_kwargs.scale": 0.02, "save_models": False,
          "algorithm_kwargs.error_feedback": ef}
    a, ra = _run(ov, tmp_path / "a", "cuda")
    b, rb = _run(ov, tmp_path / "b", "cuda")
    assert torch.equal(a.server.global_parameter, b.server.global_parameter)
    assert torch.isfinite(a.server.global_parameter).all()
    if ef:
        assert a.worker._error.abs().sum() > 0 and torch.equal(a.worker._error, b.worker._error)
    else:
        assert a.worker._error is None
    assert ra["bytes_up"] == rb["bytes_up"] == 2 * 4 * _nb(a) * 516
