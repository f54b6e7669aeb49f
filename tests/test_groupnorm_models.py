"""ResNet-GN models on the CPU path: `model_kwargs.norm: group` keeps the BatchNorm model's flat
layout, rejects what it cannot build, composes like plain torch (F.conv2d, F.group_norm, add, relu
under autograd), keeps clients independent — and makes a sample's prediction independent of the
rest of its batch, which the BatchNorm model's is not.
"""

import pytest
import torch
import torch.nn.functional as F

import gn_common as gc
from distributed_learning_simulator_amd.data.datasets import get_spec
from distributed_learning_simulator_amd.engine.params import BoundParams
from distributed_learning_simulator_amd.models.layers import GroupNorm, RunCtx
from distributed_learning_simulator_amd.models.zoo import BasicBlock, CohortModel, build_model
from distributed_learning_simulator_amd.ops import functional as Fn

GN = {"norm": "group"}


@pytest.mark.parametrize("name,ds,count", [("ResNet18", "CIFAR10", 11173962), ("Resnet50", "ImageNet", 25557032)])
def test_gn_layout_equals_bn_layout(name, ds, count):
    spec = get_spec(ds)
    bn, gn = build_model(name, spec), build_model(name, spec, GN)
    assert gn.num_params == bn.num_params == count
    assert [(e.name, e.shape, e.offset, e.init) for e in gn.layout.entries] == \
        [(e.name, e.shape, e.offset, e.init) for e in bn.layout.entries]
    kinds = {m.kind for m in gn.root.modules()}
    assert "GroupNorm" in kinds and "BatchNorm2d" not in kinds
    assert all(m.groups == 2 for m in gn.root.modules() if isinstance(m, GroupNorm))  # the default
    g32 = build_model(name, spec, {"norm": "group", "gn_groups": 32})
    assert all(m.groups == 32 for m in g32.root.modules() if isinstance(m, GroupNorm))
    assert build_model(name, spec, {"norm": "batch"}).layout.entries == bn.layout.entries


def test_norm_option_errors():
    spec = get_spec("CIFAR10")
    with pytest.raises(ValueError, match="norm must be one of"):
        build_model("ResNet18", spec, {"norm": "layer"})
    with pytest.raises(ValueError, match="gn_groups=3 does not divide"):
        build_model("ResNet18", spec, {"norm": "group", "gn_groups": 3})
    with pytest.raises(ValueError, match="not available for densenet40"):
        build_model("densenet40", spec, GN)
    build_model("densenet40", spec, {"norm": "batch"})


def _run(model, x, labels, K, theta, valid=None):
    grad = torch.zeros_like(theta)
    params = BoundParams(model.layout, theta, grad)
    ctx = RunCtx(params, valid if valid is not None else torch.full((K,), labels.shape[1], dtype=torch.int32))
    logits = model.forward(x, ctx)
    loss, _ = Fn.cross_entropy(logits, labels, ctx.valid)
    loss.sum().backward()
    return loss.detach(), grad


def test_cohort_clients_are_independent_resnet18_gn():
    """tests/test_models.py::test_cohort_clients_are_independent's check for ResNet-18-GN."""
    torch.manual_seed(0)
    spec = get_spec("CIFAR10")
    model = build_model("ResNet18", spec, GN)
    g = torch.Generator().manual_seed(1)
    theta = torch.stack([model.layout.init_flat(g), model.layout.init_flat(g)])
    H, W, C = spec.shape
    x = torch.randn(2, 4, H, W, C)
    y = torch.randint(0, spec.num_classes, (2, 4))
    loss2, grad2 = _run(model, x, y, 2, theta.clone())
    loss1, grad1 = _run(model, x[1:], y[1:], 1, theta[1:].clone())
    torch.testing.assert_close(loss2[1:], loss1, rtol=1e-4, atol=1e-5)
    scale = grad1.abs().max().item()
    assert (grad2[1:] - grad1).abs().max().item() <= 1e-2 * scale
    assert grad2.abs().sum() > 0


@pytest.mark.parametrize("cin,cout,stride", [(16, 16, 1), (16, 32, 2)], ids=["identity", "downsample"])
def test_basic_block_gn_matches_torch_autograd(cin, cout, stride):
    """One BasicBlock with GroupNorm on 8x8 inputs == F.conv2d / F.group_norm / add / relu under
    autograd: output, input gradient and every parameter gradient (the identity block routes the
    shortcut's gradient through a ResidualLink, the downsample block through its donor conv)."""
    K, B, G = 2, 3, 2
    gen = torch.Generator().manual_seed(9)
    model = CohortModel(BasicBlock(cin, cout, stride, lambda c, relu=False: GroupNorm(c, G, relu=relu)), "block",
                        "image", 0)
    layout = model.layout
    theta = torch.stack([layout.init_flat(gen) for _ in range(K)])
    for e in layout.entries:  # non-trivial γ / β
        if e.init in ("ones", "zeros"):
            theta[:, e.offset: e.offset + e.numel] += 0.3 * torch.randn(K, e.numel, generator=gen)
    x = torch.randn(K, B, 8, 8, cin, generator=gen)
    dy = torch.randn(K, B, 8 // stride, 8 // stride, cout, generator=gen)
    grad = torch.zeros_like(theta)
    ctx = RunCtx(BoundParams(layout, theta.clone(), grad), torch.full((K,), B, dtype=torch.int32))
    xa = x.clone().requires_grad_()
    out = model.forward(xa, ctx)
    out.backward(dy)
    assert (cin == cout) == (model.root.down is None)
    for k in range(K):
        t = {n: v.clone().requires_grad_() for n, v in layout.unflatten(theta[k]).items()}
        xk = x[k].permute(0, 3, 1, 2).clone().requires_grad_()

        def conv(h, name, s, pad):
            return F.conv2d(h, t[name + ".weight"].permute(0, 3, 1, 2), stride=s, padding=pad)

        def gn(h, name):
            return F.group_norm(h, G, t[name + ".weight"], t[name + ".bias"], eps=1e-5)

        h = F.relu(gn(conv(xk, "conv1", stride, 1), "bn1"))
        h = gn(conv(h, "conv2", 1, 1), "bn2")
        sc = xk if cin == cout else gn(conv(xk, "downsample.0", stride, 0), "downsample.1")
        o = F.relu(h + sc)
        o.backward(dy[k].permute(0, 3, 1, 2))
        tol = dict(rtol=1e-4)  # (test_models.py's autograd comparisons: rtol 1e-4, atol 1e-6 of the scale)
        torch.testing.assert_close(out[k].detach(), o.detach().permute(0, 2, 3, 1), atol=1e-6 * o.abs().max().item(),
                                   **tol)
        gx = xk.grad.permute(0, 2, 3, 1)
        torch.testing.assert_close(xa.grad[k], gx, atol=1e-6 * gx.abs().max().item(), **tol)
        got = layout.unflatten(grad[k])
        assert set(got) == set(t)
        for n, v in t.items():
            torch.testing.assert_close(got[n], v.grad, atol=1e-6 * v.grad.abs().max().item(), msg=n, **tol)


def _sample0_logits(norm, x, valid):
    spec = get_spec("CIFAR10")
    model = build_model("ResNet18", spec, {"norm": norm})
    theta = torch.stack([model.layout.init_flat(torch.Generator().manual_seed(s)) for s in (5, 6)])
    ctx = RunCtx(BoundParams(model.layout, theta, None), valid, training=False)
    with torch.no_grad():
        return model.forward(x, ctx)[:, 0].clone()


def test_prediction_is_independent_of_the_batch_with_group_norm():
    """Replace samples 1–3 and lower `valid` to 1: sample 0's logits are bitwise unchanged with
    `norm: group`. The same check on `norm: batch` moves them by more than 1e-3 — the property is
    GroupNorm's, not the harness's."""
    a, b = gc.batch_composition_inputs()
    full, one = torch.full((2,), 4, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    ga, gb = _sample0_logits("group", a, full), _sample0_logits("group", b, one)
    assert torch.isfinite(ga).all() and torch.equal(ga, gb)
    ba, bb = _sample0_logits("batch", a, full), _sample0_logits("batch", b, one)
    assert (ba - bb).abs().max().item() > 1e-3
