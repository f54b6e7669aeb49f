"""The server optimiser kernel (csrc/server_opt.hip) against the CPU oracle (ops/ref.py) on the MI355X: θ',
m', v' and the pre-cast x bit for bit for every rule and data kind over three chained steps, operands as
views inside guarded buffers, and two launches with the same bits."""

import os
import sys

import pytest
import torch

from distributed_learning_simulator_amd.ops import fl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_server_opt as TSO  # noqa: E402  (data kinds, the shared oracle runs, the bitwise helpers)

pytestmark = pytest.mark.gpu

RULES, KINDS, HYPER, NAN = TSO.RULES, TSO.KINDS, TSO.HYPER, TSO.NAN
_case, _oracle, _same, _bits64, _bits32, _tile = TSO._case, TSO._oracle, TSO._same, TSO._bits64, TSO._bits32, TSO._tile

# one quad; a few; less than a wave of quads; one full block of 256 quads plus one quad; several blocks
SMALL = [4, 16, 48, 1028, 4112]
GUARD = 64


def _same_on_device(a, e):
    """`_same` without the copies to the host (the large case)."""
    bits = torch.int64 if a.dtype == torch.float64 else torch.int32
    na = a.isnan()
    return a.dtype == e.dtype and torch.equal(na, e.isnan()) and torch.equal(a.view(bits)[~na], e.view(bits)[~na])


def _guarded(t, fill, P):
    """t[:P] as a view inside a wider buffer, `fill` before and after it (the view stays 32-B aligned)."""
    wide = torch.full((GUARD + P + GUARD,), fill, dtype=t.dtype, device="cuda")
    wide[GUARD : GUARD + P] = t.cuda()
    return wide, wide[GUARD : GUARD + P]


def _guards_hold(wide, fill, P):
    lo, hi = wide[:GUARD], wide[GUARD + P :]
    if fill != fill:
        return bool(lo.isnan().all() and hi.isnan().all())
    return bool((lo == fill).all() and (hi == fill).all())


def _chain(kind, rule, P, with_x=True, case=None):
    """The three chained steps on the device, operands inside guarded buffers: 7.0 around θ, m, v and x,
    NaN after target[P] (the target is passed LONGER than P: target[P:] must not be read)."""
    th0, ts, m0, v0 = case or _case(kind, P)
    lr, b1, b2, tau = HYPER[rule]
    wth, th = _guarded(th0, 7.0, P)
    wm, m = _guarded(m0, 7.0, P)
    wv, v = (None, None) if rule == "sgdm" else _guarded(v0, 7.0, P)
    wx, x = _guarded(torch.zeros(P, dtype=torch.float64), 7.0, P) if with_x else (None, None)
    out = []
    for t in ts:
        wt = torch.full((P + GUARD,), NAN, dtype=torch.float64, device="cuda")
        wt[:P] = t.cuda()
        before = wt.clone()
        assert fl.server_opt_step(th, wt, m, v, rule, lr, b1, b2, tau, x_out=x) is th
        assert torch.equal(wt.view(torch.int64), before.view(torch.int64))  # read-only
        out.append((th.clone(), m.clone(), None if v is None else v.clone(), None if x is None else x.clone()))
    assert _guards_hold(wth, 7.0, P) and _guards_hold(wm, 7.0, P)
    assert wv is None or _guards_hold(wv, 7.0, P)
    assert wx is None or _guards_hold(wx, 7.0, P)
    return out


def _check(kind, rule, P, got, want=None):
    for step, ((th, m, v, x), (eth, em, ev, ex)) in enumerate(zip(got, want or _oracle(kind, rule, P))):
        where = (kind, rule, P, step)
        assert th.is_cuda and th.dtype == torch.float32 and m.dtype == torch.float64
        assert _same(th, eth), (where, "theta", int((_bits32(th) != _bits32(eth)).sum()))
        assert _same(m, em), (where, "m", int((_bits64(m) != _bits64(em)).sum()))
        assert (v is None) == (ev is None)
        if v is not None:
            assert _same(v, ev), (where, "v", int((_bits64(v) != _bits64(ev)).sum()))
        if x is not None:
            assert _same(x, ex), (where, "x", int((_bits64(x) != _bits64(ex)).sum()))


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("kind", KINDS)
def test_hip_step_matches_oracle_bit_for_bit(hip, kind, rule):
    for P in SMALL:
        _check(kind, rule, P, _chain(kind, rule, P))
    _check(kind, rule, 1028, _chain(kind, rule, 1028, with_x=False))  # the instantiation that writes no x


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("kind", KINDS)
def test_hip_step_matches_oracle_past_the_grid_cap(hip, kind, rule):
    """One P past what the capped grid covers in one trip (cap · 256 lanes · 4 elements), plus 48: the
    grid-stride loop takes a second trip for some lanes only."""
    per_trip = hip.server_opt_max_elements()
    assert per_trip == 8192 * 256 * 4
    P = per_trip + 48
    th0, ts, m0, v0 = _case(kind, TSO.BASE)  # repeated to P on the device, and so is the oracle's result
    case = (_tile(th0.cuda(), P), [_tile(t.cuda(), P) for t in ts], _tile(m0.cuda(), P), _tile(v0.cuda(), P))
    got = _chain(kind, rule, P, case=case)
    del case
    want = _oracle(kind, rule, TSO.BASE)
    for step, (g, w) in enumerate(zip(got, want)):
        for name, a, e in zip(("theta", "m", "v", "x"), g, w):
            assert (a is None) == (e is None)
            if a is not None:
                assert _same_on_device(a, _tile(e.cuda(), P)), (kind, rule, P, step, name)


@pytest.mark.parametrize("rule", RULES)
def test_hip_two_launches_give_the_same_bits(hip, rule):
    for kind, P in (("gauss", 4112), ("wide", 1028), ("poison", 48)):
        a, b = _chain(kind, rule, P), _chain(kind, rule, P)
        for (th, m, v, x), (th2, m2, v2, x2) in zip(a, b):
            assert torch.equal(_bits32(th), _bits32(th2)) and torch.equal(_bits64(m), _bits64(m2))
            assert torch.equal(_bits64(x), _bits64(x2))
            assert v is None or torch.equal(_bits64(v), _bits64(v2))


def test_hip_operand_errors_raise_before_any_launch(hip):
    P = 16
    th = torch.zeros(P, device="cuda")
    t, m, v = (torch.zeros(P, dtype=torch.float64, device="cuda") for _ in range(3))
    wide = torch.zeros(P + 8, dtype=torch.float64, device="cuda")
    hp = ("adam", 0.01, 0.9, 0.99, 1e-3)
    for ops in ((th, wide[1 : 1 + P], m, v), (th, t, wide[1 : 1 + P], v), (th, t, m, wide[2 : 2 + P]),
                (torch.zeros(P + 4, device="cuda")[1 : 1 + P], t, m, v), (th, t[:12], m, v), (th, t.cpu(), m, v),
                (th, t, m, None), (torch.zeros(6, device="cuda"), t, m, v)):
        with pytest.raises(ValueError, match="server_opt_step"):
            fl.server_opt_step(*ops, *hp)
    with pytest.raises(ValueError, match="tau"):
        fl.server_opt_step(th, t, m, v, "yogi", 0.01, 0.9, 0.99, 0.0)
    with pytest.raises(ValueError, match="rule"):
        fl.server_opt_step(th, t, m, v, "lamb", 0.01, 0.9, 0.99, 1e-3)
    torch.cuda.synchronize()
    assert (th == 0).all() and (m == 0).all() and (v == 0).all()
