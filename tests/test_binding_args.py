"""The keyword-only launch bindings (csrc/bindings.cpp Args) refuse a bad call before anything
launches: positional arguments, a missing required key, an unknown key, an unknown field of a
dict-valued key. No GPU needed: importing the extension does not touch the device, and no case
here passes a complete argument set, so every call ends in the argument reader."""

import importlib

import pytest
import torch  # noqa: F401  (the HIP runtime is loaded through torch)

from distributed_learning_simulator_amd.ops import build

# binding -> (a required key, a dict-valued key or None)
BINDINGS = {
    "conv_nt": ("x_cs", None),
    "conv_dgrad": ("w_cs", "bnb"),
    "conv_tn": ("dw_cs", "sgd"),
    "halo_wgrad": ("xm", "sgd"),
    "bn_fwd": ("eps", None),
    "bn_bwd": ("ws", None),
    "dense_dgrad_bn": ("g_cs", None),
    "dense_wgrad": ("part", None),
    "conv_halo_bn_fwd": ("wsplit", None),
    "conv_halo_bn_dense_fwd": ("creal", None),
}


@pytest.fixture(scope="module")
def C():
    build.build()
    return importlib.import_module("distributed_learning_simulator_amd._dls_hip")


def test_bn_bwd_conv_tn_variant_binding_is_gone(C):
    assert not hasattr(C, "conv_tn_bn_bwd")  # conv_tn takes the bnb_* keys instead


@pytest.mark.parametrize("name", BINDINGS)
def test_positional_call_is_refused(C, name):
    with pytest.raises(TypeError):
        getattr(C, name)(0)
    with pytest.raises(TypeError):
        getattr(C, name)(0, K=1, s=0)


@pytest.mark.parametrize("name", BINDINGS)
def test_missing_required_key_is_named(C, name):
    required = BINDINGS[name][0]
    with pytest.raises(TypeError, match=rf"{name}\(\): missing required argument\(s\).* '{required}'"):
        getattr(C, name)(K=1, s=0)
    # ... and only the missing ones: a key that was passed is not reported
    with pytest.raises(TypeError) as e:
        getattr(C, name)(**{required: 1})
    assert f"'{required}'" not in str(e.value) and "'K'" in str(e.value)


@pytest.mark.parametrize("name", BINDINGS)
def test_unknown_key_is_named(C, name):
    with pytest.raises(TypeError, match=rf"{name}\(\):.*unexpected argument\(s\).* 'no_such_operand'"):
        getattr(C, name)(K=1, s=0, no_such_operand=0)


@pytest.mark.parametrize("name", [n for n, (_, sub) in BINDINGS.items() if sub])
def test_dict_valued_key_with_unknown_field_is_refused(C, name):
    sub = BINDINGS[name][1]
    with pytest.raises(TypeError, match=rf"{name}\({sub}=\):.*unexpected argument\(s\) 'bogus'"):
        getattr(C, name)(K=1, s=0, **{sub: {"bogus": 1}})
    with pytest.raises(TypeError, match=f"'{sub}' must be a dict or None"):
        getattr(C, name)(K=1, s=0, **{sub: (1, 2, 3)})


def test_wrong_type_is_named(C):
    with pytest.raises(TypeError, match=r"conv_tn\(\): argument 'M' has the wrong type"):
        C.conv_tn(M="many")
    with pytest.raises(TypeError, match=r"conv_tn\(sgd=\): argument 'wd' has the wrong type"):
        C.conv_tn(sgd={"wd": None})
