"""ops.fusion: the BatchNorm output forms, the deferral base and the tensor tag record (CPU)."""

import gc
import weakref

import pytest
import torch

from distributed_learning_simulator_amd.ops import functional as Fn
from distributed_learning_simulator_amd.ops import fusion
from distributed_learning_simulator_amd.ops.fusion import BNOut, Deferral, Tags, tag, tags


def test_bn_out_values_and_rules():
    assert sorted(BNOut) == [0, 1, 2, 3, 4, 5] and len(BNOut) == 6
    assert BNOut(2) == 2 and BNOut(2) is BNOut.PLANES  # (integer call sites keep working)
    down = {3: 2, 4: 0, 5: 1}
    for form in BNOut:
        assert form.applied_now == down.get(int(form), int(form))
        assert isinstance(form.applied_now, BNOut)
        assert form.applied_now.applied_now is form.applied_now
        assert form.reads_planes == (int(form) not in (0, 4))


def test_functional_reexports_the_vocabulary():
    for name in ("ResidualLink", "MaskedGrad", "BNStats", "BNBwdLink", "DeferredBN", "DeferredStemBN",
                 "DeferredRes", "DeferredBNBwd", "BNOut", "stem_defer_count", "res_fold_count",
                 "bn_bwd_defer_count", "bn_bwd_f32_defer_count", "bn_bwd_parts_count"):
        assert getattr(Fn, name) is getattr(fusion, name), name
    assert fusion.stem_defer_count.keys() == {"conv", "res", "materialized"}
    assert fusion.res_fold_count.keys() == {"folded", "materialized"}
    assert fusion.bn_bwd_defer_count.keys() == fusion.bn_bwd_f32_defer_count.keys() == {"wgrad", "materialized"}
    assert fusion.bn_bwd_parts_count.keys() == {"used", "none", "fallback"}


class _Stub(Deferral):
    __slots__ = ("calls",)

    def __init__(self, count):
        super().__init__(count)
        self.calls = 0

    def _apply(self):
        self.calls += 1


def test_deferral_materialize_applies_and_counts_once():
    count = {"x": 0, "materialized": 0}
    d = _Stub(count)
    assert d.pending
    d.materialize()
    d.materialize()
    assert d.calls == 1 and not d.pending and count == {"x": 0, "materialized": 1}


def test_deferral_taken_leaves_nothing_to_materialize():
    count = {"x": 0, "materialized": 0}
    d = _Stub(count)
    d.taken("x")
    d.materialize()
    assert d.calls == 0 and not d.pending and count == {"x": 1, "materialized": 0}
    quiet = _Stub(None)  # (a deferral that counts nothing: DeferredBN)
    quiet.taken("x")
    quiet.materialize()
    assert quiet.calls == 0 and not quiet.pending


def test_untagged_tensor_reads_as_defaults_and_cannot_be_written():
    t = torch.zeros(2)
    rec = tags(t)
    assert rec is tags(None) is tags(torch.ones(1))  # (the one shared default)
    assert [getattr(rec, f) for f in Tags.__slots__] == [None, False, None, None, None, None, False]
    for field in ("planes_only", "plane_only"):
        with pytest.raises(AttributeError):
            setattr(rec, field, True)
    assert tags(t).planes_only is False and not hasattr(t, "_dls")


def test_unknown_tag_field_raises():
    t = torch.zeros(2)
    with pytest.raises(AttributeError):
        tags(t).plane_only
    with pytest.raises(AttributeError):
        tag(t, plane_only=True)
    rec = tag(t, planes_only=True)
    with pytest.raises(AttributeError):
        rec.plane_only
    with pytest.raises(AttributeError):
        rec.plane_only = False
    assert tags(t) is rec and rec.planes_only is True and rec.owned is False


def test_aliases_share_one_record():
    a = torch.zeros(2, 3)
    b = a.view(6)
    rec = tag(a, planes_only=True)
    assert tag(b, rec) is rec and tags(b).planes_only
    tags(b).planes_only = False
    assert tags(a).planes_only is False
    tag(a, owned=True)
    assert tags(b).owned and tags(a) is tags(b)
    tag(b, planes_only=True)
    with pytest.raises(RuntimeError, match="planes-only"):
        Fn._require_fp32(a, "reader")


def test_deferred_bn_bwd_operands_die_with_the_delivered_tensor():
    """The fp32 BN-backward deferral as _BN.backward builds it: the delivered tensor's record holds the
    deferral, which holds the untagged buffer. No reference cycle: with the cyclic collector off,
    the operands are freed as soon as the delivered tensor is, taken or not."""
    on = gc.isenabled()
    gc.disable()
    try:
        dy, x, coef, dx = torch.zeros(2, 6, 8), torch.zeros(2, 6, 8), torch.zeros(2, 8, 3), torch.empty(2, 6, 8)
        dxo = dx.reshape(2, 2, 3, 8)
        tag(dxo, planes_only=True, bn_bwd=fusion.DeferredBNBwd(dy, x, None, coef, None, dx, f32=True))
        assert not hasattr(dx, "_dls") and tags(dxo).bn_bwd.out is dx
        alive = [weakref.ref(t) for t in (dy, x, coef, dx)]
        del dy, x, coef, dx
        assert all(r() is not None for r in alive)
        del dxo
        assert all(r() is None for r in alive)
    finally:
        if on:
            gc.enable()
