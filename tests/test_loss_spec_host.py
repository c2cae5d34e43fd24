"""LossSpec on the host: validation, the detection of the reference's spec, the f64 restatement of tests/loss_spec_cases.py
against the oracle and against its own closed-form gradient, and the argument contracts of the uclstm_loss_spec_* entry points
(nothing is launched here)."""
import ctypes as C
import dataclasses
import inspect
import math

import pytest
import torch

import boundary_cases as BC
import loss_spec_cases as LC
from oracle import unet_oracle as O

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops
from unet_convlstm_amd.loss import LossSpec

SMALL_CASES = [c for c in LC.CASES if c not in LC.LARGE_CASES]


@pytest.mark.parametrize("kwargs", [
    dict(point="l3"), dict(point=None), dict(point="L1"),
    dict(point="huber", delta=0.0), dict(point="huber", delta=-1.0), dict(point="huber", delta=math.inf),
    dict(point="huber", delta=math.nan), dict(point="huber", delta="1"),
    dict(weight_gain=-0.5), dict(weight_gain=math.inf), dict(weight_gain=math.nan), dict(weight_gain=None),
    dict(weight_power=0), dict(weight_power=5), dict(weight_power=2.0), dict(weight_power=True), dict(weight_power="3"),
    dict(grad_weight=-1e-3), dict(grad_weight=math.inf), dict(grad_weight=math.nan),
    dict(eps=0.0), dict(eps=-1e-8), dict(eps=math.nan),
], ids=str)
def test_invalid_fields_raise_at_construction(kwargs):
    with pytest.raises(ValueError):
        LossSpec(**kwargs)


def test_defaults_presets_and_the_reference_detection():
    s = LossSpec()
    assert dataclasses.astuple(s) == ("l1", 1.0, 4.0, 3, 0.005, 1e-8)
    assert LossSpec.reference() == s and s.is_reference and LossSpec.reference().is_reference
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.point = "l2"
    mse = LossSpec.masked_mse()
    assert (mse.point, mse.weight_gain, mse.grad_weight, mse.eps) == ("l2", 0.0, 0.0, 1e-6) and LossSpec.masked_mse(eps=1e-3).eps == 1e-3
    for field, value in (("point", "l2"), ("delta", 2.0), ("weight_gain", 4.5), ("weight_power", 2), ("grad_weight", 0.0), ("eps", 1e-6)):
        assert not dataclasses.replace(s, **{field: value}).is_reference, field
    assert not any(sp.is_reference for name, sp in LC.SPECS.items() if name != "reference") and LC.SPECS["reference"].is_reference
    assert LossSpec(point="l1", delta=-3.0).delta == -3.0            # delta is Huber's alone
    assert U.LossSpec is LossSpec and "LossSpec" in U.__all__


def test_the_descriptor_mirrors_the_header_struct():
    assert C.sizeof(L.LossSpecDesc) == 32
    assert [f[0] for f in L.LossSpecDesc._fields_] == ["point", "weight_power", "delta", "weight_gain", "grad_term", "reserved_"]
    hdr = open(L.HEADER_PATH).read()
    body = hdr[hdr.index("typedef struct uclstm_loss_spec {"):hdr.index("} uclstm_loss_spec;")]
    for line in ("int32_t point;", "int32_t weight_power;", "float delta;", "float weight_gain;", "int32_t grad_term;", "int32_t reserved[3];"):
        assert line in body, line
    d = ops.loss_spec_desc(LossSpec(point="huber", delta=0.5, weight_gain=2.5, weight_power=2, grad_weight=0.0))
    assert (d.point, d.weight_power, d.delta, d.weight_gain, d.grad_term, list(d.reserved_)) == (L.LOSS_POINT_HUBER, 2, 0.5, 2.5, 0, [0, 0, 0])
    assert ops.loss_spec_desc(LossSpec()).grad_term == 1 and ops.loss_spec_desc(LossSpec()).point == L.LOSS_POINT_L1
    assert ops.loss_spec_desc(LossSpec(point="l2")).point == L.LOSS_POINT_L2
    syms = set(L.header_symbols())
    for name in ("uclstm_loss_spec_fwd", "uclstm_loss_spec_fwd_ordered", "uclstm_loss_spec_bwd"):
        assert name in syms and name in L._PROTOS and name not in L._ALL_F16_TWINS, name


def test_the_loss_keyword_is_on_every_public_signature():
    def params(fn):
        return list(inspect.signature(fn).parameters.items())

    assert [k for k, _ in params(U.compute_loss)] == ["y_pred", "y", "mask", "use_mask", "spec"]
    assert [k for k, _ in params(U.train_step)][-2:] == ["clip_norm", "loss"]
    assert [k for k, _ in params(U.train_one_epoch)][-2:] == ["ddp", "loss"]
    assert [k for k, _ in params(U.evaluate)][-2:] == ["tta", "loss"]
    assert [k for k, _ in params(U.evaluate_report)][-3:] == ["tta", "loss", "report_kwargs"]
    assert [k for k, _ in params(U.GraphedTrainStep.__init__)][-2:] == ["warmup", "loss"]
    for fn in (U.train_step, U.train_one_epoch, U.evaluate, U.evaluate_report, U.GraphedTrainStep.__init__):
        assert dict(params(fn))["loss"].default is None
    assert dict(params(U.compute_loss))["spec"].default is None
    x = torch.zeros(1, 1, 1, 2, 2)
    with pytest.raises(TypeError):
        U.compute_loss(x, x, None, False, spec="l2")
    with pytest.raises(TypeError):
        U.train_step(None, None, x, x, loss=dict(point="l2"))
    with pytest.raises(TypeError):
        U.evaluate(None, [], "cpu", None, loss="l2")
    with pytest.raises(TypeError):
        U.evaluate_report(None, [], "cpu", None, loss=1.0)
    with pytest.raises(TypeError):
        U.train_one_epoch(None, [], None, "cpu", None, loss=LossSpec)
    with pytest.raises(TypeError):
        U.GraphedTrainStep(None, None, x, x, loss="l2")


@pytest.mark.parametrize("case", [c for c in SMALL_CASES if min(c[1:]) > 1], ids=str)
def test_loss_ref_at_the_default_spec_is_the_oracle(case):
    """The same formula in the same precision: 1e-12 relative, masked, unmasked and with the mask ignored."""
    planes, H, W = case
    for masked, use_mask in ((True, True), (False, True), (True, False)):
        yp, y, mask = LC.inputs(case, masked)
        shape = (planes, 1, 1, H, W)
        yp5, y5, m5 = yp.double().view(shape), y.double().view(shape), (mask.double().view(shape) if masked else None)
        want = float(O.compute_loss(yp5, y5, m5, use_mask=use_mask))
        for got in (float(LC.loss_ref(yp5, y5, m5, use_mask, LossSpec())), float(LC.loss_ref(yp, y, mask, use_mask, LossSpec()))):
            assert math.isfinite(want) and want > 0 and abs(got - want) <= 1e-12 * want, (case, masked, use_mask, got, want)


@pytest.mark.parametrize("case", SMALL_CASES, ids=str)
def test_loss_ref_at_masked_mse_is_the_overfit_check_loss(case):
    yp, y, mask = LC.inputs(case, True)
    yp, y, mask = yp.double(), y.double(), mask.double()
    want = float(((yp - y) ** 2 * mask).sum() / (mask.sum() + 1e-6))
    got = float(LC.loss_ref(yp, y, mask, True, LossSpec.masked_mse()))
    assert math.isfinite(got) and abs(got - want) <= 1e-12 * want, (got, want)
    assert float(LC.loss_ref(yp, y, None, True, LossSpec.masked_mse())) == pytest.approx(float(((yp - y) ** 2).mean()), rel=1e-12)


@pytest.mark.parametrize("name", list(LC.SPECS), ids=str)
def test_autograd_of_loss_ref_is_the_closed_form(name):
    """Every spec on every small case and one large one, masked and unmasked: d loss_ref / d y_pred == loss_bwd_ref with the
    coefficients the host layer forms.  A plane without cells (H or W = 1) has no unmasked loss unless the gradient term is off."""
    spec = LC.SPECS[name]
    for case in SMALL_CASES + LC.LARGE_CASES[:1]:
        planes, H, W = case
        for masked in (False, True):
            if min(H, W) == 1 and not masked and spec.grad_weight != 0:
                continue
            yp, y, mask = LC.inputs(case, masked)
            leaf = yp.double().clone().requires_grad_(True)
            loss = LC.loss_ref(leaf, y, mask, masked, spec)
            assert bool(torch.isfinite(loss))
            loss.backward()
            c1, c2 = LC.coefs_ref(y, mask, masked, spec)
            ref, mag = LC.loss_bwd_ref(yp, y, mask, spec, c1, c2)
            torch.testing.assert_close(ref, leaf.grad, rtol=1e-12, atol=1e-15, msg=lambda s: f"{name} {case} {masked}: {s}")
            assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
            sums, counts = LC.sums_ref(yp, y, mask, spec)
            d1, d2 = ((float(sums[1]) + spec.eps, float(sums[3]) + spec.eps) if masked else (float(counts[0]), float(counts[2])))
            want = float(sums[0]) / d1 + (spec.grad_weight * float(sums[2]) / d2 if spec.grad_weight != 0 else 0.0)
            assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)


def test_closed_form_at_the_reference_spec_is_boundary_cases():
    for case in SMALL_CASES:
        for masked in (False, True):
            yp, y, mask = LC.inputs(case, masked)
            a, am = LC.loss_bwd_ref(yp, y, mask, LossSpec(), *BC.LOSS_COEFS)
            b, bm = BC.loss_bwd_ref(yp, y, mask, *BC.LOSS_COEFS)
            assert torch.equal(a, b) and bool((am <= bm).all())          # |sign(0)| = 0 here, 1 there


def test_spec_entry_points_check_their_arguments_before_launch():
    """UCLSTM_E_BADARG from the arguments alone: every pointer is a non-null address that is never dereferenced because nothing is
    launched; each call differs from an accepted one in the one thing named."""
    P = C.c_void_p(1 << 20)
    big = 1 << 16
    lib = L.lib

    def desc(**kw):
        base = dict(point=L.LOSS_POINT_HUBER, weight_power=3, delta=1.0, weight_gain=4.0, grad_term=1)
        base.update(kw)
        return C.byref(L.LossSpecDesc(base["point"], base["weight_power"], base["delta"], base["weight_gain"], base["grad_term"]))

    def fwd(spec, yp=P, y=P, sums=P, planes=3, H=8, W=8):
        return lib.uclstm_loss_spec_fwd(spec, yp, y, None, sums, planes, H, W, None)

    def fwd_ordered(spec, yp=P, y=P, partials=P, sums=P, planes=3, H=8, W=8):
        return lib.uclstm_loss_spec_fwd_ordered(spec, yp, y, None, partials, sums, 0, planes, H, W, None)

    def bwd(spec, yp=P, y=P, coefs=P, grad=P, planes=3, H=8, W=8):
        return lib.uclstm_loss_spec_bwd(spec, yp, y, None, coefs, grad, planes, H, W, None)

    bad_specs = [None, desc(point=-1), desc(point=3), desc(weight_power=0), desc(weight_power=5), desc(delta=0.0), desc(delta=-1.0),
                 desc(delta=math.inf), desc(delta=math.nan), desc(weight_gain=-1.0), desc(weight_gain=math.inf),
                 desc(weight_gain=math.nan)]
    for call in (fwd, fwd_ordered, bwd):
        for i, spec in enumerate(bad_specs):
            assert call(spec) == -1, (call.__name__, i)
        for kw in (dict(yp=None), dict(y=None), dict(planes=0), dict(H=0), dict(W=-1), dict(planes=2, H=big, W=big // 4)):
            assert call(desc(), **kw) == -1, (call.__name__, kw)
    assert fwd(desc(), sums=None) == -1
    assert fwd_ordered(desc(), sums=None) == -1 and fwd_ordered(desc(), partials=None) == -1
    assert bwd(desc(), coefs=None) == -1 and bwd(desc(), grad=None) == -1
