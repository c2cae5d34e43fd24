"""WeightedLossSpec on the host: validation, presets, the detection of the plain and of the reference's spec, the f64 restatement
of tests/loss_weight_cases.py against loss_spec_cases.py and against its own closed-form gradient, and the argument contracts of
the uclstm_loss_spec_*_pw entry points (nothing is launched here)."""
import ctypes as C
import dataclasses
import math

import pytest
import torch

import loss_spec_cases as LC
import loss_weight_cases as WC

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops
from unet_convlstm_amd.loss import LossSpec, WeightedLossSpec

PW_SYMBOLS = ("uclstm_loss_spec_fwd_pw", "uclstm_loss_spec_fwd_ordered_pw", "uclstm_loss_spec_bwd_pw")


@pytest.mark.parametrize("kwargs", [
    dict(frame_weights=()), dict(frame_weights=[]), dict(channel_weights=()),
    dict(frame_weights=(0.0, 0.0)), dict(channel_weights=(0,)),
    dict(frame_weights=(1.0, -0.5)), dict(channel_weights=(-1e-9, 1.0)),
    dict(frame_weights=(1.0, math.inf)), dict(frame_weights=(math.nan, 1.0)), dict(channel_weights=(1.0, math.inf)),
    dict(frame_weights=(True, 1.0)), dict(channel_weights=(1.0, False)),
    dict(frame_weights=("1", 1.0)), dict(frame_weights=(None, 1.0)), dict(channel_weights=(1.0, 1j)),
    dict(frame_weights=1.0), dict(frame_weights="11"), dict(channel_weights={1.0, 2.0}), dict(frame_weights=torch.ones(3)),
    dict(point="l3", frame_weights=(1.0,)), dict(weight_power=5), dict(eps=0.0),
], ids=str)
def test_invalid_weights_raise_at_construction(kwargs):
    with pytest.raises(ValueError):
        WeightedLossSpec(**kwargs)


def test_fields_storage_hashing_and_the_plain_spec_unchanged():
    assert dataclasses.astuple(LossSpec()) == ("l1", 1.0, 4.0, 3, 0.005, 1e-8)
    assert [f.name for f in dataclasses.fields(LossSpec)] == ["point", "delta", "weight_gain", "weight_power", "grad_weight", "eps"]
    s = WeightedLossSpec()
    assert isinstance(s, LossSpec) and dataclasses.astuple(s) == ("l1", 1.0, 4.0, 3, 0.005, 1e-8, None, None)
    assert [f.name for f in dataclasses.fields(s)][-2:] == ["frame_weights", "channel_weights"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.frame_weights = (1.0,)
    a = WeightedLossSpec(frame_weights=[0, 0.25, 1.5], channel_weights=[1, 0.3, 2])
    assert a.frame_weights == (0.0, 0.25, 1.5) and a.channel_weights == (1.0, 0.3, 2.0)
    assert all(type(v) is float for v in a.frame_weights + a.channel_weights)
    b = WeightedLossSpec(frame_weights=(0.0, 0.25, 1.5), channel_weights=(1.0, 0.3, 2.0))
    assert a == b and hash(a) == hash(b) and len({a, b, s}) == 2
    assert a != dataclasses.replace(a, channel_weights=None) and a != dataclasses.replace(a, point="l2")
    assert U.WeightedLossSpec is WeightedLossSpec and "WeightedLossSpec" in U.__all__


def test_base_and_the_reference_detection():
    s = WeightedLossSpec()
    assert type(s.base) is LossSpec and s.base == LossSpec() and s.is_reference and not s.weighted
    h = WeightedLossSpec(point="huber", delta=2.0, weight_power=1, weight_gain=0.75, grad_weight=0.02, eps=1e-6, frame_weights=(0, 1))
    assert type(h.base) is LossSpec and h.base == LossSpec(point="huber", delta=2.0, weight_power=1, weight_gain=0.75, grad_weight=0.02, eps=1e-6)
    assert not WeightedLossSpec(point="l2").is_reference and type(WeightedLossSpec(point="l2").base) is LossSpec
    # weights, even all ones, are weights: such a spec takes the weighted entry points and is not the reference's
    for kw in (dict(frame_weights=(1.0, 1.0)), dict(channel_weights=(1.0,)), dict(frame_weights=(0.0, 1.0), channel_weights=(2.0,))):
        w = WeightedLossSpec(**kw)
        assert w.weighted and not w.is_reference and w.base.is_reference
    assert LossSpec().is_reference and LossSpec() != WeightedLossSpec()          # another class: never equal to a plain spec


def test_presets():
    b = WeightedLossSpec.burn_in(5, 2)
    assert b.frame_weights == (0.0, 0.0, 1.0, 1.0, 1.0) and b.channel_weights is None and b.base.is_reference
    assert WeightedLossSpec.burn_in(4, 0).frame_weights == (1.0,) * 4
    m = WeightedLossSpec.burn_in(3, 1, point="l2", grad_weight=0.0, channel_weights=(0, 0, 1))
    assert (m.point, m.grad_weight, m.frame_weights, m.channel_weights) == ("l2", 0.0, (0.0, 1.0, 1.0), (0.0, 0.0, 1.0))
    k = WeightedLossSpec.last_frames(5, 2, point="huber", delta=0.5)
    assert k.frame_weights == (0.0, 0.0, 0.0, 1.0, 1.0) and (k.point, k.delta) == ("huber", 0.5)
    assert WeightedLossSpec.last_frames(3, 3).frame_weights == (1.0,) * 3
    assert WeightedLossSpec.last_frames(6, 2) == WeightedLossSpec.burn_in(6, 4)
    for bad in (lambda: WeightedLossSpec.burn_in(3, 3), lambda: WeightedLossSpec.burn_in(3, -1), lambda: WeightedLossSpec.burn_in(0, 0),
                lambda: WeightedLossSpec.burn_in(3.0, 1), lambda: WeightedLossSpec.last_frames(3, 0),
                lambda: WeightedLossSpec.last_frames(3, 4), lambda: WeightedLossSpec.last_frames(3, True)):
        with pytest.raises(ValueError):
            bad()


def test_plane_weights_are_f64_products_and_name_a_length_mismatch():
    s = WeightedLossSpec(frame_weights=(0.0, 0.25, 1.5), channel_weights=(1.0, 0.3, 2.0))
    assert s.plane_weights(3, 3) == [f * c for f in (0.0, 0.25, 1.5) for c in (1.0, 0.3, 2.0)]
    assert torch.equal(torch.tensor(s.plane_weights(3, 3), dtype=torch.float64).float(), WC.table(s, 3, 3))
    assert WeightedLossSpec(frame_weights=(2.0, 3.0)).plane_weights(2, 3) == [2.0] * 3 + [3.0] * 3
    assert WeightedLossSpec(channel_weights=(2.0, 3.0)).plane_weights(2, 2) == [2.0, 3.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="frame_weights.*3.*T = 4"):
        s.plane_weights(4, 3)
    with pytest.raises(ValueError, match="channel_weights.*3.*Cy = 1"):
        s.plane_weights(3, 1)
    # the table needs [B,T,Cy,H,W]; the check comes before anything touches a device
    with pytest.raises(ValueError, match="B,T,Cy,H,W"):
        ops.plane_weight_table(s, torch.zeros(3, 3, 4, 4))
    with pytest.raises(ValueError, match="frame_weights"):
        ops.plane_weight_table(s, torch.zeros(1, 2, 3, 4, 4))


def test_the_loss_keyword_accepts_the_weighted_spec():
    from unet_convlstm_amd.loss import check_spec
    s = WeightedLossSpec.burn_in(3, 1)
    assert check_spec(s) is s
    with pytest.raises(TypeError):
        check_spec((0.0, 1.0))


def test_the_entry_points_are_declared_bound_and_exported():
    syms = set(L.header_symbols())
    for name in PW_SYMBOLS:
        assert name in syms and name in L._PROTOS and name not in L._ALL_F16_TWINS and name + "_f16" not in syms, name
        assert callable(getattr(L.lib, name))
    assert L.lib.uclstm_abi_version() == 16 and "#define UCLSTM_ABI_VERSION 16" in open(L.HEADER_PATH).read()
    assert len(L._PROTOS["uclstm_loss_spec_fwd_pw"]) == len(L._PROTOS["uclstm_loss_spec_fwd_bc"]) + 2
    assert len(L._PROTOS["uclstm_loss_spec_fwd_ordered_pw"]) == len(L._PROTOS["uclstm_loss_spec_fwd_ordered_bc"]) + 2
    assert len(L._PROTOS["uclstm_loss_spec_bwd_pw"]) == len(L._PROTOS["uclstm_loss_spec_bwd_bc"]) + 2


def test_pw_entry_points_check_their_arguments_before_launch():
    """UCLSTM_E_BADARG from the arguments alone: every pointer is a non-null address that is never dereferenced because nothing is
    launched; each call differs from an accepted one in the one thing named."""
    P = C.c_void_p(1 << 20)
    big = 1 << 16
    lib = L.lib

    def desc(**kw):
        base = dict(point=L.LOSS_POINT_HUBER, weight_power=3, delta=1.0, weight_gain=4.0, grad_term=1)
        base.update(kw)
        return C.byref(L.LossSpecDesc(base["point"], base["weight_power"], base["delta"], base["weight_gain"], base["grad_term"]))

    def fwd(spec, yp=P, y=P, mask=P, pw=P, period=6, sums=P, planes=12, H=8, W=8, mask_div=3):
        return lib.uclstm_loss_spec_fwd_pw(spec, yp, y, mask, pw, period, sums, planes, H, W, mask_div, None)

    def fwd_ordered(spec, yp=P, y=P, mask=P, pw=P, period=6, partials=P, sums=P, planes=12, H=8, W=8, mask_div=3):
        return lib.uclstm_loss_spec_fwd_ordered_pw(spec, yp, y, mask, pw, period, partials, sums, 0, planes, H, W, mask_div, None)

    def bwd(spec, yp=P, y=P, mask=P, pw=P, period=6, coefs=P, grad=P, planes=12, H=8, W=8, mask_div=3):
        return lib.uclstm_loss_spec_bwd_pw(spec, yp, y, mask, pw, period, coefs, grad, planes, H, W, mask_div, None)

    bad_specs = [None, desc(point=-1), desc(point=3), desc(weight_power=0), desc(weight_power=5), desc(delta=0.0), desc(delta=-1.0),
                 desc(delta=math.inf), desc(delta=math.nan), desc(weight_gain=-1.0), desc(weight_gain=math.inf),
                 desc(weight_gain=math.nan)]
    for call in (fwd, fwd_ordered, bwd):
        for i, spec in enumerate(bad_specs):
            assert call(spec) == -1, (call.__name__, i)
        for kw in (dict(yp=None), dict(y=None), dict(planes=0), dict(H=0), dict(W=-1), dict(planes=2, period=2, H=big, W=big // 4),
                   dict(pw=None), dict(period=0), dict(period=-6), dict(period=5), dict(period=24), dict(planes=13),
                   dict(mask=None), dict(mask=None, mask_div=2), dict(mask_div=0), dict(mask_div=-1)):
            assert call(desc(), **kw) == -1, (call.__name__, kw)
    assert fwd(desc(), sums=None) == -1
    assert fwd_ordered(desc(), sums=None) == -1 and fwd_ordered(desc(), partials=None) == -1
    assert bwd(desc(), coefs=None) == -1 and bwd(desc(), grad=None) == -1


# ---------------------------------------------------------------------------------------------
# the f64 restatement
# ---------------------------------------------------------------------------------------------
def small_runs():
    return [(n, c, k) for n, c, k in WC.runs() if c in WC.SMALL_CASES]


@pytest.mark.parametrize("case", WC.SMALL_CASES, ids=str)
def test_loss_ref_at_all_ones_is_the_plain_loss_ref(case):
    B, T, Cy, H, W = case
    for name in (WC.NOGRAD_SPECS if min(H, W) == 1 else tuple(LC.SPECS)):
        plain = LC.SPECS[name]
        fields = dataclasses.asdict(plain)
        ones = [WeightedLossSpec(**fields), WeightedLossSpec(**fields, frame_weights=(1.0,) * T),
                WeightedLossSpec(**fields, frame_weights=(1,) * T, channel_weights=(1,) * Cy)]
        for kind in WC.MASKS:
            if kind == "broadcast" and Cy == 1:
                continue
            yp, y, mask = WC.inputs(case, kind)
            for use_mask in (True, False):
                want = float(LC.loss_ref(yp, y, None if mask is None else mask.expand_as(y), use_mask, plain))
                for spec in ones:
                    got = float(WC.loss_ref(yp, y, mask, use_mask, spec))
                    assert math.isfinite(want) and want > 0 and abs(got - want) <= 1e-12 * want, (name, case, kind, use_mask, got, want)


def test_scaling_all_weights_leaves_the_loss_unchanged():
    case = (2, 3, 3, 5, 7)
    a = WC.spec_for("huber2_p1", case)
    b = dataclasses.replace(a, frame_weights=tuple(4.0 * v for v in a.frame_weights), channel_weights=tuple(0.5 * v for v in a.channel_weights))
    for kind in WC.MASKS:
        yp, y, mask = WC.inputs(case, kind)
        la, lb = float(WC.loss_ref(yp, y, mask, True, a)), float(WC.loss_ref(yp, y, mask, True, b))
        assert abs(la - lb) <= 1e-9 * la and abs(la - float(LC.loss_ref(yp, y, None if mask is None else mask.expand_as(y), True, a.base))) > 1e-3 * la


@pytest.mark.parametrize("name,case,kind", small_runs(), ids=str)
def test_autograd_of_loss_ref_is_the_closed_form(name, case, kind):
    spec = WC.spec_for(name, case)
    yp, y, mask = WC.inputs(case, kind)
    masked = mask is not None
    leaf = yp.double().clone().requires_grad_(True)
    loss = WC.loss_ref(leaf, y, mask, True, spec)
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    loss.backward()
    c1, c2 = WC.coefs_ref(y, mask, True, spec)
    ref, mag = WC.loss_bwd_ref(yp, y, mask, spec, c1, c2)
    torch.testing.assert_close(ref, leaf.grad, rtol=1e-12, atol=1e-15, msg=lambda s: f"{name} {case} {kind}: {s}")
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    # a plane of weight 0 has no gradient, and the loss is the quotient of the sums
    q = WC.table(spec, case[1], case[2]).view(1, case[1], case[2], 1, 1).expand(case)
    assert bool((ref[q == 0] == 0).all()) and bool((q == 0).any()) and float(ref[q > 0].abs().max()) > 0
    sums, counts = WC.sums_ref(yp, y, mask, spec)
    d1, d2 = (float(v) for v in WC.denominators(y, mask, True, spec))
    if masked:
        assert d1 == float(sums[1]) + spec.eps and (spec.grad_weight == 0 or d2 == float(sums[3]) + spec.eps)
    want = float(sums[0]) / d1 + (spec.grad_weight * float(sums[2]) / d2 if spec.grad_weight != 0 else 0.0)
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("kind", WC.MASKS, ids=str)
@pytest.mark.parametrize("name", ["reference", "masked_mse", "huber2_p1"], ids=str)
def test_burn_in_is_the_plain_loss_of_the_later_frames(name, kind):
    case = (2, 3, 3, 5, 7)
    plain = LC.SPECS[name]
    yp, y, mask = WC.inputs(case, kind)
    for k in (0, 1, 2):
        spec = WeightedLossSpec.burn_in(3, k, **dataclasses.asdict(plain))
        for use_mask in (True, False):
            m = None if mask is None else mask.expand_as(y)[:, k:]
            want = float(LC.loss_ref(yp[:, k:], y[:, k:], m, use_mask, plain))
            got = float(WC.loss_ref(yp, y, mask, use_mask, spec))
            assert abs(got - want) <= 1e-12 * want, (name, kind, k, use_mask, got, want)
    last = WeightedLossSpec.last_frames(3, 1, **dataclasses.asdict(plain))
    want = float(LC.loss_ref(yp[:, 2:], y[:, 2:], None if mask is None else mask.expand_as(y)[:, 2:], True, plain))
    assert abs(float(WC.loss_ref(yp, y, mask, True, last)) - want) <= 1e-12 * want
