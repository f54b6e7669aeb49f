"""The benchmark's command line: `--steps` sets the number of timed rounds, the result line
carries `ms_per_step`, `--dump-outputs DIR` writes the last timed round's results as float
.npy files that repeat exactly from run to run, and `--full` is accepted. Runs the smallest
workload (FedAvg, 4 clients, MLP, MNIST-shaped) on the CPU executor."""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    env = dict(os.environ, DLS_FORCE_CPU="1", PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
           "--workload", "fedavg_mlp_mnist", *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), r.stderr


def test_dump_outputs_repeat_and_result_line(tmp_path):
    a, err = _bench("--dump-outputs", str(tmp_path / "a"))
    b, _ = _bench("--dump-outputs", str(tmp_path / "b"), "--full")
    # one progress line per round: no warm-up round, exactly --steps timed ones
    assert err.count("[bench] warmup round") == 0 and err.count("[bench] timed round") == 2
    for out in (a, b):
        assert out["steps"] == 2 and out["warmup"] == 0 and out["unit"] == "rounds/s"
        assert out["higher_is_better"] is True and out["dtype"] == "fp32"
        assert out["ms_per_step"] > 0
        # value (rounds/s) and ms_per_step describe the same timed rounds
        assert abs(out["value"] * out["ms_per_step"] / 1000.0 - 1.0) < 1e-9
    assert a["metric"] == b["metric"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["global_parameters.npy", "round_metrics.npy"]
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all()
        np.testing.assert_array_equal(x, y)  # seeded inputs, CPU executor: bit-identical runs
        total += x.nbytes
    assert total <= 64 * 2**20
    theta = np.load(tmp_path / "a" / "global_parameters.npy")
    assert theta.dtype == np.float32 and theta.ndim == 1 and np.abs(theta).max() > 0
    loss, acc = np.load(tmp_path / "a" / "round_metrics.npy")
    assert acc == a["test_accuracy_last_round"] and loss > 0


def test_dump_samples_a_large_model(tmp_path, monkeypatch):
    """A model above the element budget is written as a fixed, seeded sample (same positions
    every run), a smaller one whole; the budget keeps the files under 64 MB."""
    import torch

    import bench

    assert bench.DUMP_MAX_ELEMENTS * 4 + 16 <= 64 * 2**20
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", 1000)
    d = str(tmp_path)
    small = torch.arange(1000, dtype=torch.float32)
    bench.dump_outputs(d, small, {"test_loss": 1.5, "test_accuracy": 0.25})
    np.testing.assert_array_equal(np.load(os.path.join(d, "global_parameters.npy")), small.numpy())
    np.testing.assert_array_equal(np.load(os.path.join(d, "round_metrics.npy")), [1.5, 0.25])
    big = torch.arange(5000, dtype=torch.float32)
    bench.dump_outputs(d, big, {})
    s1 = np.load(os.path.join(d, "global_parameters.npy"))
    bench.dump_outputs(d, big, {})
    s2 = np.load(os.path.join(d, "global_parameters.npy"))
    assert s1.shape == (1000,) and s1.dtype == np.float32
    np.testing.assert_array_equal(s1, s2)
    assert (np.diff(s1) > 0).all()  # positions are distinct and ascending
