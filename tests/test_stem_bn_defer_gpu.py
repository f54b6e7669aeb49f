"""The ResNet stem BatchNorm without standalone apply passes.

Forward (OPTIONS.bn_stem_defer, ops.functional DeferredStemBN): the stem BN's two readers apply it
themselves — layer1.0.conv1 in its halo loader, layer1.0.bn2 in its residual fold (bn_fwd res_coef
+ res_relu). Backward (OPTIONS.bn_bwd_in_wgrad_f32, DeferredBNBwdF32): the stem conv's fp32 weight
gradient applies the BN backward in its dY loader (conv_wgrad bn_bwd=). Both recompute the
expressions of the standalone passes, so everything here compares with torch.equal.
"""

import pytest
import torch

from distributed_learning_simulator_amd import options
from distributed_learning_simulator_amd.ops import ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5  # (fp32 kernels against fp64, tests/test_kernels_f32_gpu.py)


def _d(t):
    return t.detach().cpu().double()


# ------------------------------------------------------------------ 1. bn_fwd with res_relu
@pytest.mark.parametrize("with_mask", [True, False])
def test_bn_fwd_res_relu_fold_bitwise(hip, with_mask):
    """out = relu(bn(x2) + relu(bn(x1))) with the inner BN applied first (its fp32 output read back as
    the residual) and folded (its raw input + (scale, shift) + res_relu): y, ReLU bits and planes are
    equal bit for bit — full, ragged mid-image and empty clients; training and inference forms."""
    torch.manual_seed(0)
    K, B, H, C = 3, 3, 8, 64
    R = B * H * H
    vr = torch.tensor([R, H * H + 36, 0], dtype=torch.int32, device=DEV)
    x1, x2 = torch.randn(K, R, C, device=DEV), torch.randn(K, R, C, device=DEV) * 1.5 + 0.2
    g1, b1 = torch.rand(K, C, device=DEV) + 0.5, torch.randn(K, C, device=DEV) * 0.3
    g2, b2 = torch.rand(K, C, device=DEV) + 0.5, torch.randn(K, C, device=DEV) * 0.3
    y1 = hip.bn_fwd(x1, g1, b1, vr, relu=True)[0]
    a = hip.bn_fwd(x2, g2, b2, vr, relu=True, residual=y1, with_mask=with_mask, planes=1)
    coef1 = hip.bn_coef(x1, g1, b1, vr)[0]
    b = hip.bn_fwd(x2, g2, b2, vr, relu=True, residual=x1, with_mask=with_mask, planes=1, res_coef=coef1,
                   res_relu=True)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[-1], b[-1])  # split planes
    if with_mask:
        assert a[3] is not None and torch.equal(a[3], b[3])
        assert 0 < int((a[3][0] != 0).sum()) and int((a[3][0] == 0xFF).sum()) < a[3][0].numel()  # (both bit values)
    assert not a[0][2].any() and not a[0][1, int(vr[1]):].any()  # rows past the valid ones stay zero
    assert a[0][0].abs().max() > 0


# ------------------------------------------------- 2. fp32 TN weight gradient, BN-backward loader
# K, B, H, splits, kernel size: the stem shape of the issue (M = 180, not a multiple of the 32-row K
# tile; the split rule gives pixel reductions under 256 rows one split), B = 9 (M = 324: two splits,
# the second ragged), and a 1x1 conv (R = 8: the 64x64 tile, the other one with this loader)
WGRAD_CASES = [(3, 5, 6, 1, 3), (3, 9, 6, 2, 3), (3, 9, 6, 2, 1)]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", WGRAD_CASES)
def test_wgrad_bn_bwd_loader_bitwise(hip, case, relu):
    """dW of a 3x3 / pad-1 (or 1x1) conv of an 8-channel (zero-padded RGB) input with 64 output channels whose
    dY is a BatchNorm(+ReLU) input gradient: built in the TN kernel's dY loader it equals the separate
    BN-backward apply pass followed by conv_wgrad bit for bit, is reproducible run to run and within
    1e-5 of fp64. dy is nonzero on the rows past the valid ones (full, 100, 0), which must not count."""
    K, B, H, min_splits, ks = case
    pad = ks // 2
    torch.manual_seed(1)
    C, Co = 8, 64
    M = B * H * H
    vr = torch.tensor([M, 100, 0], dtype=torch.int32, device=DEV)
    x = torch.randn(K, B, H, H, C, device=DEV)
    x[..., 3:] = 0
    xb = torch.randn(K, M, Co, device=DEV) * 1.3 + 0.1
    dy = torch.randn(K, M, Co, device=DEV)
    mask = torch.randint(0, 256, (K, M, Co // 8), dtype=torch.uint8, device=DEV) if relu else None
    mean, rstd = torch.randn(K, Co, device=DEV) * 0.1, torch.rand(K, Co, device=DEV) + 0.5
    gamma = torch.rand(K, Co, device=DEV) + 0.5
    assert hip._C.conv_tn_splitk(K, Co, ks * ks * C, M, C, hip.tn_f32_variant, 1) >= min_splits
    assert hip.conv_wgrad_bn_bwd_ok(x.shape, Co, ks, ks)

    # separate apply pass, then the plain weight gradient
    dx, _ = hip.bn_bwd(dy, xb, None, mean, rstd, gamma, vr, relu, None, None, False, relu_mask=mask)
    gw_sep = torch.empty(K, Co, ks, ks, C, device=DEV)
    hip.conv_wgrad(dx.view(K, B, H, H, Co), x, gw_sep, 1, pad)
    # coefficients only, applied in the loader
    coef = torch.empty(K, Co, 3, device=DEV)
    hip.bn_bwd(dy, xb, None, mean, rstd, gamma, vr, relu, None, None, False, relu_mask=mask, coef_out=coef)
    shape_only = torch.empty(K, B, H, H, Co, device=DEV)
    runs = []
    for _ in range(2):
        gw = torch.full((K, Co, ks, ks, C), float("nan"), device=DEV)
        hip.conv_wgrad(shape_only, x, gw, 1, pad, bn_bwd=(dy, xb, mask, coef, vr))
        runs.append(gw)
    assert torch.equal(runs[0], gw_sep)
    assert torch.equal(runs[0], runs[1])

    # fp64: dX = a·(dy·bit) + e·x + d on the valid rows, zero past them
    cf = _d(coef)
    g = _d(dy)
    if relu:
        bits = ((mask.cpu().view(K, M, Co // 8, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).reshape(K, M, Co)
        g = g * bits.double()
    dx64 = cf[:, None, :, 0] * g + cf[:, None, :, 2] * _d(xb) + cf[:, None, :, 1]
    rows = torch.arange(M)[None, :, None] < vr.cpu()[:, None, None]
    dx64 = torch.where(rows, dx64, torch.zeros((), dtype=torch.float64))
    exp = ref.conv_wgrad(dx64.view(K, B, H, H, Co), _d(x), (K, Co, ks, ks, C), 1, pad)
    err = (_d(runs[0]) - exp).abs().max().item()
    mag = exp.abs().max().item() + 1e-12
    print(f"wgrad bn_bwd loader {case} relu={relu}: rel err {err / mag:.3g}")
    assert err <= TOL * mag, f"rel err {err / mag:.3g} > {TOL}"
    assert not runs[0][2].any() and runs[0][1].abs().max() > 0  # (the empty client's dW is zero)


# ------------------------------------------------------------------------------ 3, 4. sessions
_OV = {"round": 2, "epoch": 1, "worker_number": 4, "model_name": "ResNet18", "dataset_kwargs.scale": 0.01,
       "learning_rate": 0.05}
_runs: dict = {}


def _session(tmp_path_factory, **opts):
    """One 2-round ResNet-18 session (ragged last batches) under `opts`, run once per module:
    (global parameters, evaluation losses, the counters it left)."""
    from distributed_learning_simulator_amd.config import load_config
    from distributed_learning_simulator_amd.ops import backend, functional as Fn
    from distributed_learning_simulator_amd.parallel.comm import Comm
    from distributed_learning_simulator_amd.session import Session

    key = tuple(sorted(opts.items()))
    if key not in _runs:
        d = tmp_path_factory.mktemp("stem")
        args = ["--config-name", "fed_avg/cifar10.yaml"] + [f"++fed_avg.{k}={v}" for k, v in _OV.items()]
        args += [f"++fed_avg.save_dir={d}", "++fed_avg.log_level=WARNING", "++fed_avg.save_models=False"]
        Fn.stem_defer_count.update(conv=0, res=0, materialized=0)
        Fn.bn_bwd_f32_defer_count.update(wgrad=0, materialized=0)
        with options.override(**opts):
            sess = Session(load_config(args), comm=Comm(device=torch.device("cuda")))
            assert backend.using_hip(sess.trainer.buffers.theta) and sess.compute_dtype == torch.float32
            res = sess.run()
        perf = res["performance"]
        _runs[key] = (sess.server.global_parameter.clone(), [perf[k]["test_loss"] for k in sorted(perf)],
                      dict(Fn.stem_defer_count), dict(Fn.bn_bwd_f32_defer_count))
    return _runs[key]


def _same(a, b):
    assert torch.equal(a[0], b[0])
    assert a[1] == b[1]


def test_resnet18_defaults_take_both_fused_paths(hip, tmp_path_factory):
    """With the defaults both readers of the stem BN apply it themselves and the stem conv's weight
    gradient applies its backward: nothing is materialised."""
    assert options.OPTIONS.bn_stem_defer and options.OPTIONS.bn_bwd_in_wgrad_f32
    _, _, fwd, bwd = _session(tmp_path_factory)
    assert fwd["conv"] > 0 and fwd["res"] > 0 and fwd["materialized"] == 0, fwd
    assert bwd["wgrad"] > 0 and bwd["materialized"] == 0, bwd


def test_resnet18_stem_bn_defer_bitwise(hip, tmp_path_factory):
    """OPTIONS.bn_stem_defer on / off: the same global model and evaluation losses, bit for bit."""
    on = _session(tmp_path_factory)
    off = _session(tmp_path_factory, bn_stem_defer=False)
    assert off[2] == {"conv": 0, "res": 0, "materialized": 0}, off[2]
    _same(on, off)


def test_resnet18_bn_bwd_in_wgrad_f32_bitwise(hip, tmp_path_factory):
    """OPTIONS.bn_bwd_in_wgrad_f32 on / off: the same global model and evaluation losses."""
    on = _session(tmp_path_factory)
    off = _session(tmp_path_factory, bn_bwd_in_wgrad_f32=False)
    assert off[3] == {"wgrad": 0, "materialized": 0}, off[3]
    _same(on, off)


@pytest.mark.parametrize("opt", ["bn_fused_halo", "halo_wgrad"])
def test_resnet18_stem_readers_fall_back_bitwise(hip, tmp_path_factory, opt):
    """With the conv reader unable to fuse (bn_fused_halo off: it materialises planes + bits while the
    residual reader still folds) or its weight gradient unable to apply the BN (halo_wgrad off: the
    fused forward writes the planes), the session equals the run with both new options off. The
    all-off run keeps the fallback switch as it is: halo_wgrad off moves layers 1-3's weight
    gradients to another kernel with another summation order, which changes the bits by itself.
    bn_fused_halo is bitwise neutral, so that run also equals the plain all-off session."""
    all_off = _session(tmp_path_factory, bn_stem_defer=False, bn_bwd_in_wgrad_f32=False, **{opt: False})
    fb = _session(tmp_path_factory, **{opt: False})
    assert fb[2]["res"] > 0, fb[2]
    if opt == "bn_fused_halo":
        assert fb[2]["conv"] == 0 and fb[2]["materialized"] > 0, fb[2]
    else:
        assert fb[2]["conv"] > 0 and fb[2]["materialized"] == 0, fb[2]
    _same(fb, all_off)
    if opt == "bn_fused_halo":
        _same(fb, _session(tmp_path_factory, bn_stem_defer=False, bn_bwd_in_wgrad_f32=False))


# ------------------------------------------------------------ 5. a net that must not take the mode
def test_bottleneck_resnet_keeps_the_stem_apply(hip):
    """ResNet-50's first block has a downsample shortcut: the stem BN has no residual reader, so the
    two-reader mode is not requested (a training epoch of two clients runs; the counter stays 0)."""
    from distributed_learning_simulator_amd.data.datasets import create_dataset_collection
    from distributed_learning_simulator_amd.engine.trainer import CohortTrainer, HyperParameter
    from distributed_learning_simulator_amd.models.zoo import build_model
    from distributed_learning_simulator_amd.ops import functional as Fn

    dev = torch.device("cuda:0")
    dc = create_dataset_collection("CIFAR10", {"n_train": 64, "n_test": 32}, 0, dev, torch.float32, image_channels=8)
    model = build_model("ResNet50", dc.spec)
    trainer = CohortTrainer(model, dc, HyperParameter(epoch=1, batch_size=8, learning_rate=0.05), dev, torch.float32,
                            capacity=2)
    trainer.load_global(model.layout.init_flat(torch.Generator().manual_seed(0)).to(dev), 2)
    Fn.stem_defer_count.update(conv=0, res=0, materialized=0)
    stats = trainer.train(trainer.build_schedule([torch.arange(0, 8), torch.arange(8, 20)], 1, seed=0))
    torch.cuda.synchronize()
    loss, _ = stats.epoch_metrics(0)
    assert torch.isfinite(loss).all(), loss
    assert Fn.stem_defer_count == {"conv": 0, "res": 0, "materialized": 0}, Fn.stem_defer_count
