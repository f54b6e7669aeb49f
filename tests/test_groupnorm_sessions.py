"""ResNet-18 with GroupNorm (`model_kwargs.norm: group`) end to end on the MI355X: the FedAvg session
against the CPU oracle, bitwise reproducibility with HIP-graph steps and ragged last batches, and the
property GroupNorm is there for — a sample's prediction does not depend on the rest of its batch.
"""

import pytest
import torch

import gn_common as gc
from distributed_learning_simulator_amd.config import load_config
from distributed_learning_simulator_amd.data.datasets import get_spec
from distributed_learning_simulator_amd.engine.params import BoundParams
from distributed_learning_simulator_amd.models.layers import RunCtx
from distributed_learning_simulator_amd.models.zoo import build_model
from distributed_learning_simulator_amd.ops import backend
from distributed_learning_simulator_amd.parallel.comm import Comm
from distributed_learning_simulator_amd.session import Session

pytestmark = pytest.mark.gpu

# the settings of tests/test_gpu_sessions.py::test_fedavg_resnet18_matches_cpu, with GroupNorm
OV = {"round": 2, "epoch": 1, "worker_number": 4, "model_name": "ResNet18", "model_kwargs.norm": "group",
      "dataset_kwargs.scale": 0.01, "learning_rate": 0.01}


def _run(overrides, tmp_path, device):
    args = ["--config-name", "fed_avg/cifar10.yaml"] + [f"++fed_avg.{k}={v}" for k, v in overrides.items()]
    args += [f"++fed_avg.save_dir={tmp_path}", "++fed_avg.log_level=WARNING", "++fed_avg.save_models=False"]
    sess = Session(load_config(args), comm=Comm(device=torch.device(device)))
    if device == "cuda":
        assert backend.using_hip(sess.trainer.buffers.theta) and sess.compute_dtype == torch.float32
    kinds = {m.kind for m in sess.model.root.modules()}
    assert "GroupNorm" in kinds and "BatchNorm2d" not in kinds
    return sess, sess.run()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def _losses(res):
    perf = res["performance"]
    return [perf[k]["test_loss"] for k in sorted(perf)]


@pytest.fixture(scope="module")
def gpu_run(hip, tmp_path_factory):
    """The GPU session both tests below compare against (run once)."""
    return _run(OV, tmp_path_factory.mktemp("gn_gpu"), "cuda")


def test_fedavg_resnet18_gn_matches_cpu(gpu_run, tmp_path):
    import os

    gs, gr = gpu_run
    cs, cr = _run(OV, tmp_path / "cpu", "cpu")
    gl, cl = _losses(gr), _losses(cr)
    g, c = gs.server.global_parameter, cs.server.global_parameter
    if os.environ.get("DLS_PRINT_TOL") == "1":
        print(f"TOL resnet18-gn: loss diffs {[abs(a - b) for a, b in zip(gl, cl)]} param rel {_rel(g, c):.3g}")
    assert len(gl) == 2 and torch.isfinite(g).all()
    # What separates the GPU from the CPU oracle is the split-bf16 GEMMs' ≈2⁻¹⁶ per-product error against
    # the CPU's fp32, amplified by local SGD over the rounds, as in test_fedavg_resnet18_matches_cpu.
    # Measured (DLS_PRINT_TOL=1): loss diffs 4.9e-4 / 7.8e-4 (rounds 1 / 2), parameters 7.0e-5 relative;
    # the bounds are about 4× that. The parameters agree more closely than the BatchNorm model's (1.9e-4,
    # bound 8e-4), the round-1 test loss less closely (BatchNorm: 1.4e-4, bound 6e-4). We attribute the
    # latter to the evaluation: a BatchNorm divides by statistics pooled over a whole test batch, in which
    # the GEMM error of single samples averages out, whereas each GroupNorm statistic is one sample's own
    # (4,096 values per group in layer4) and passes that sample's error on to its logits.
    assert abs(gl[0] - cl[0]) < 2e-3, (gl, cl)
    assert max(abs(a - b) for a, b in zip(gl, cl)) < 3e-3, (gl, cl)
    assert _rel(g, c) < 3e-4


def test_fedavg_resnet18_gn_is_bitwise_reproducible(gpu_run, tmp_path):
    """The same run again gives the same bits: HIP-graph steps on, ragged last batches included (125
    samples per client in batches of 64); the GroupNorm dγ / dβ are per-sample rows folded in order."""
    gs, gr = gpu_run
    bs, br = _run(OV, tmp_path / "again", "cuda")
    assert torch.equal(bs.server.global_parameter, gs.server.global_parameter) and _losses(br) == _losses(gr)


def _sample0_logits(norm, x, valid):
    model = build_model("ResNet18", get_spec("CIFAR10"), {"norm": norm})
    theta = torch.stack([model.layout.init_flat(torch.Generator().manual_seed(s)) for s in (5, 6)]).cuda()
    x8 = torch.nn.functional.pad(x, (0, 5)).cuda()  # (RGB stored zero-padded to 8 channels, as the sessions do)
    ctx = RunCtx(BoundParams(model.layout, theta, None), valid.cuda(), training=False)
    with torch.no_grad():
        out = model.forward(x8, ctx)
    assert backend.using_hip(theta)
    return out[:, 0].clone()


def test_prediction_is_independent_of_the_batch_on_the_gpu(hip):
    """tests/test_groupnorm_models.py's batch-composition check through the native kernels: bitwise
    for `norm: group`, off by more than 1e-3 for `norm: batch`."""
    a, b = gc.batch_composition_inputs()
    full, one = torch.full((2,), 4, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    ga, gb = _sample0_logits("group", a, full), _sample0_logits("group", b, one)
    assert torch.isfinite(ga).all() and torch.equal(ga, gb)
    ba, bb = _sample0_logits("batch", a, full), _sample0_logits("batch", b, one)
    assert (ba - bb).abs().max().item() > 1e-3
