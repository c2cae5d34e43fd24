"""The per-plane-weight loss kernels (uclstm_loss_spec_fwd_pw / _fwd_ordered_pw / _bwd_pw) at the C ABI against the f64
restatement of tests/loss_weight_cases.py and against the plain kernels, and WeightedLossSpec through compute_loss, train_step
and GraphedTrainStep.

Bounds (the inputs lie on the 1/64 grid of loss_spec_cases.py; the weights are one more f32 multiplication per term):
  * gradient: |grad - ref| <= (weight_power + 7) * 2^-24 * mag, mag = q (|c1| |rho'| w m + |c2| sum|gradient terms|)
  * each forward sum (non-negative f32 terms, added in f64): |sum - ref| <= ((weight_power + 5) * 2^-24 + count * 2^-52) * ref
  * compute_loss: with e the forward bound, |loss - ref| <= (2 e / (1 - e) + 2^-24 + 2^-50) * ref; the coefficients are off by at most
    dc = e / (1 - e) + 2 * 2^-24 relatively, so |grad - ref| <= ((weight_power + 7) * 2^-24 * (1 + dc) + dc) * mag
    (as tests/test_gpu_loss_spec.py derives them; the unmasked denominators are exact f64 products of the f32 table)
Outputs are pre-filled with NaN and every element is compared.
"""
import contextlib
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_cases as BC
import loss_spec_cases as LC
import loss_weight_cases as WC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import engine, ops
    from unet_convlstm_amd.loss import LossSpec, WeightedLossSpec

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
F32_UNIT = WC.F32_UNIT


def p_(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    L.check(getattr(L.lib, name)(*args, ops._stream()), name)


def nan_dev(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def mask_div_of(case, kind):
    return case[2] if kind == "broadcast" else 1


def on_dev(case, kind):
    yp, y, mask = WC.inputs(case, kind)
    return yp.to(DEV), y.to(DEV), (None if mask is None else mask.to(DEV))


def table_dev(spec, case):
    return WC.table(spec, case[1], case[2]).to(DEV)


def check_bound(got, ref, bound, what):
    """|got - ref| <= bound at every element (got finite everywhere)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: elements not written"
    d = (got - ref).abs()
    worst = float((d / (bound + 1e-300)).max())
    print(f"[parity] {what}: worst |err| / bound {worst:.3f} (<= 1), max |err| {float(d.max()):.3e} over {d.numel()} elements")
    bad = int((d > bound).sum())
    assert bad == 0, f"{what}: {bad} of {d.numel()} elements beyond the bound (worst {worst:.3f} x)"


def check_sums(got, ref, counts, spec, what):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: sums not written"
    for k in range(4):
        bound = WC.fwd_rel_bound(spec, counts[k]) * float(ref[k])
        err = abs(float(got[k]) - float(ref[k]))
        print(f"[parity] {what} sums[{k}]: |err| {err:.3e}, bound {bound:.3e}, value {float(ref[k]):.6e}")
        assert err <= bound, f"{what}: sums[{k}] = {float(got[k])!r}, f64 {float(ref[k])!r}, |err| {err:.3e} > {bound:.3e}"
    if spec.grad_weight == 0:
        assert float(got[2]) == 0.0 and float(got[3]) == 0.0, f"{what}: gradient sums {got[2:].tolist()} without a gradient term"


def label(name, case, kind):
    return f"{name} {case} mask {kind} ({'V4' if WC.vectorised(name, case) else 'V1'})"


@contextlib.contextmanager
def loss_calls():
    """The names of the uclstm_loss_* entry points called inside the block, in order (the row-count query left out)."""
    calls = []
    names = [n for n in L._PROTOS if n.startswith("uclstm_loss_") and not n.endswith("_rows")]
    saved = {n: getattr(L.lib, n) for n in names}
    try:
        for n in names:
            setattr(L.lib, n, (lambda f, k: lambda *a: (calls.append(k), f(*a))[1])(saved[n], n))
        yield calls
    finally:
        for n in names:
            setattr(L.lib, n, saved[n])


def fwd_ordered_pw(desc, ypd, yd, md, q, case, mask_div, accumulate=0, start=None):
    planes, H, W = WC.flat(case)
    rows = int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W))
    partials, sums = nan_dev((rows, 4), F64), (nan_dev((4,), F64) if start is None else start.to(DEV))
    call("uclstm_loss_spec_fwd_ordered_pw", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(q), q.numel(), p_(partials), p_(sums), accumulate,
         planes, H, W, mask_div)
    return partials.cpu().numpy(), sums.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# 1. C ABI against f64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,kind", WC.runs(), ids=str)
def test_pw_bwd_against_f64(name, case, kind):
    spec, (planes, H, W) = WC.spec_for(name, case), WC.flat(case)
    yp, y, mask = WC.inputs(case, kind)
    ypd, yd, md = on_dev(case, kind)
    desc, q = ops.loss_spec_desc(spec), table_dev(spec, case)
    cd = torch.tensor(BC.LOSS_COEFS, dtype=F32, device=DEV)
    grad = nan_dev(case, F32)
    call("uclstm_loss_spec_bwd_pw", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(q), q.numel(), p_(cd), p_(grad), planes, H, W,
         mask_div_of(case, kind))
    c1, c2 = (float(v) for v in cd.cpu().double())
    ref, mag = WC.loss_bwd_ref(yp, y, mask, spec, c1, c2)
    check_bound(grad, ref, WC.n_bwd(spec) * F32_UNIT * mag, f"loss_spec_bwd_pw {label(name, case, kind)}")


@pytest.mark.parametrize("name,case,kind", WC.runs(), ids=str)
def test_pw_fwd_sums_against_f64_atomic_and_ordered(name, case, kind):
    spec, (planes, H, W) = WC.spec_for(name, case), WC.flat(case)
    yp, y, mask = WC.inputs(case, kind)
    ypd, yd, md = on_dev(case, kind)
    desc, q, mask_div = ops.loss_spec_desc(spec), table_dev(spec, case), mask_div_of(case, kind)
    ref, counts = WC.sums_ref(yp, y, mask, spec)
    sums = torch.zeros(4, dtype=F64, device=DEV)
    call("uclstm_loss_spec_fwd_pw", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(q), q.numel(), p_(sums), planes, H, W, mask_div)
    check_sums(sums, ref, counts, spec, f"loss_spec_fwd_pw {label(name, case, kind)}")
    # the ordered form: the in-order sum of its rows, the same bits from a second call, accumulate adds to what is there
    what = f"loss_spec_fwd_ordered_pw {label(name, case, kind)}"
    prt, got = fwd_ordered_pw(desc, ypd, yd, md, q, case, mask_div)
    assert prt.shape[0] == min(1024, (planes * H * W + 255) // 256)
    assert np.isfinite(prt).all() and np.isfinite(got).all(), f"{what}: partial rows or sums not written"
    acc = np.zeros(4)
    for r in range(prt.shape[0]):
        acc = acc + prt[r]
    assert got.tobytes() == acc.tobytes(), f"{what}: {got} is not the in-order sum {acc}"
    check_sums(torch.from_numpy(got), ref, counts, spec, what)
    prt2, got2 = fwd_ordered_pw(desc, ypd, yd, md, q, case, mask_div)
    assert prt.tobytes() == prt2.tobytes() and got.tobytes() == got2.tobytes(), f"{what}: two launches differ"
    base = np.array([0.5, 1.5, 2.5, 3.5])
    _, got3 = fwd_ordered_pw(desc, ypd, yd, md, q, case, mask_div, accumulate=1, start=torch.from_numpy(base.copy()))
    for r in range(prt.shape[0]):
        base = base + prt[r]
    assert got3.tobytes() == base.tobytes(), f"{what} accumulate=1"


# ---------------------------------------------------------------------------------------------
# 2. C ABI against the plain kernels: a table of ones, planes of weight 0 and of weight 1
# ---------------------------------------------------------------------------------------------
def plain_ordered_and_bwd(desc, ypd, yd, md, cd, case, mask_div):
    """partials, sums and grad of uclstm_loss_spec_fwd_ordered / _bwd (mask per plane or NULL) or their _bc forms."""
    planes, H, W = WC.flat(case)
    rows = int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W))
    partials, sums, grad = nan_dev((rows, 4), F64), nan_dev((4,), F64), nan_dev(case, F32)
    if mask_div > 1:
        call("uclstm_loss_spec_fwd_ordered_bc", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(partials), p_(sums), 0, planes, H, W, mask_div)
        call("uclstm_loss_spec_bwd_bc", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(cd), p_(grad), planes, H, W, mask_div)
    else:
        call("uclstm_loss_spec_fwd_ordered", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(partials), p_(sums), 0, planes, H, W)
        call("uclstm_loss_spec_bwd", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(cd), p_(grad), planes, H, W)
    return partials.cpu().numpy(), sums.cpu().numpy(), grad.cpu()


ONES_RUNS = [(n, c, k) for n, c, k in WC.runs() if n in LC.LARGE_SPECS]


@pytest.mark.parametrize("name,case,kind", ONES_RUNS, ids=str)
def test_a_table_of_ones_gives_the_bits_of_the_plain_kernels(name, case, kind):
    spec, (planes, H, W) = LC.SPECS[name], WC.flat(case)
    ypd, yd, md = on_dev(case, kind)
    desc, mask_div = ops.loss_spec_desc(spec), mask_div_of(case, kind)
    cd = torch.tensor(BC.LOSS_COEFS, dtype=F32, device=DEV)
    prt0, sums0, grad0 = plain_ordered_and_bwd(desc, ypd, yd, md, cd, case, mask_div)
    assert np.isfinite(prt0).all() and bool(torch.isfinite(grad0).all())
    for period in sorted({1, case[1] * case[2], planes}):
        q = torch.ones(period, dtype=F32, device=DEV)
        prt, sums = fwd_ordered_pw(desc, ypd, yd, md, q, case, mask_div)
        grad = nan_dev(case, F32)
        call("uclstm_loss_spec_bwd_pw", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(q), period, p_(cd), p_(grad), planes, H, W, mask_div)
        what = f"{label(name, case, kind)} period {period}"
        assert prt.tobytes() == prt0.tobytes() and sums.tobytes() == sums0.tobytes(), f"{what}: ordered partials / sums differ"
        assert grad.cpu().numpy().tobytes() == grad0.numpy().tobytes(), f"{what}: bwd differs"


@pytest.mark.parametrize("name,case,kind", ONES_RUNS, ids=str)
def test_zero_planes_have_no_gradient_and_unit_planes_the_plain_bits(name, case, kind):
    B, T, Cy, H, W = case
    spec, planes = LC.SPECS[name], B * T * Cy
    ypd, yd, md = on_dev(case, kind)
    desc, mask_div = ops.loss_spec_desc(spec), mask_div_of(case, kind)
    cd = torch.tensor(BC.LOSS_COEFS, dtype=F32, device=DEV)
    _, _, grad0 = plain_ordered_and_bwd(desc, ypd, yd, md, cd, case, mask_div)
    q = (torch.arange(T * Cy) * 7 % 5 < 3).float()                   # zeros and ones in a pattern of period 5: none of T or Cy
    assert 0 < int(q.sum()) < q.numel()
    grad = nan_dev(case, F32)
    qd = q.to(DEV)
    call("uclstm_loss_spec_bwd_pw", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(qd), q.numel(), p_(cd), p_(grad), planes, H, W, mask_div)
    grad, q5 = grad.cpu(), q.view(1, T, Cy, 1, 1).expand(case)
    assert bool((grad[q5 == 0] == 0).all()), "a plane of weight 0 has a gradient"
    assert torch.equal(grad[q5 == 1].view(torch.int32), grad0[q5 == 1].view(torch.int32)), "a plane of weight 1 differs from the plain kernel"
    assert float(grad0[q5 == 0].abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# 3. compute_loss(spec=WeightedLossSpec(...))
# ---------------------------------------------------------------------------------------------
HOST_SPECS = ("reference", "masked_mse", "huber2_p1", "huber_nograd")
HOST_CASES = [(2, 2, 3, 3, 5), (2, 3, 3, 8, 8), (2, 3, 3, 5, 7)]
MODES = [("plane", True), ("broadcast", True), ("broadcast", False), ("none", True)]


@pytest.mark.parametrize("kind,use_mask", MODES, ids=str)
@pytest.mark.parametrize("case", HOST_CASES, ids=str)
@pytest.mark.parametrize("name", HOST_SPECS, ids=str)
@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "ordered"])
def test_compute_loss_with_weights_against_f64(deterministic, name, case, kind, use_mask):
    spec = WC.spec_for(name, case)
    yp, y, mask = WC.inputs(case, kind)
    ypd, yd, md = on_dev(case, kind)
    leaf = ypd.clone().requires_grad_(True)
    ops.LAUNCH_LOG = []
    try:
        with loss_calls() as calls, ops.deterministic(deterministic):
            loss = U.compute_loss(leaf, yd, md, use_mask, spec=spec)
            loss.backward()
        log = list(ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
    assert log == [("reduce", "loss_fwd_ordered" if deterministic else "loss_fwd")]
    assert calls == ["uclstm_loss_spec_fwd_ordered_pw" if deterministic else "uclstm_loss_spec_fwd_pw", "uclstm_loss_spec_bwd_pw"], calls
    m_eff = mask if use_mask else None
    want = float(WC.loss_ref(yp, y, mask, use_mask, spec))
    e = WC.fwd_rel_bound(spec, yp.numel())
    tol = (2 * e / (1 - e) + F32_UNIT + 2.0 ** -50) * want
    what = f"compute_loss {name} {case} mask {kind} use_mask={use_mask} {'ordered' if deterministic else 'atomic'}"
    print(f"[parity] {what}: loss {float(loss)!r}, f64 {want!r}, |err| {abs(float(loss) - want):.3e}, bound {tol:.3e}")
    assert loss.dtype == F32 and abs(float(loss) - want) <= tol, what
    c1, c2 = WC.coefs_ref(y, m_eff, use_mask, spec)
    ref, mag = WC.loss_bwd_ref(yp, y, m_eff, spec, c1, c2)
    dc = e / (1 - e) + 2 * F32_UNIT
    check_bound(leaf.grad, ref, (WC.n_bwd(spec) * F32_UNIT * (1 + dc) + dc) * mag, f"{what} gradient")


def test_a_weighted_spec_without_weights_is_its_base_launch_for_launch():
    case = (2, 3, 3, 8, 8)
    ypd, yd, md = on_dev(case, "broadcast")
    got = []
    for spec in (None, WeightedLossSpec(), LossSpec(point="l2"), WeightedLossSpec(point="l2")):
        leaf = ypd.clone().requires_grad_(True)
        with loss_calls() as calls, ops.deterministic():
            loss = U.compute_loss(leaf, yd, md, True, spec=spec)
            loss.backward()
        got.append((loss.detach().cpu(), leaf.grad.cpu(), calls))
    for a, b in ((got[0], got[1]), (got[2], got[3])):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and not any(n.endswith("_pw") for n in b[2])
    # and without a mask the reference's own kernels
    with loss_calls() as calls:
        U.compute_loss(ypd, yd, None, True, spec=WeightedLossSpec())
    assert calls == ["uclstm_loss_fwd"], calls


def test_wrong_lengths_and_4d_input_raise():
    case = (2, 3, 3, 8, 8)
    ypd, yd, md = on_dev(case, "broadcast")
    with pytest.raises(ValueError, match="frame_weights.*2.*T = 3"):
        U.compute_loss(ypd, yd, md, True, spec=WeightedLossSpec(frame_weights=(0.0, 1.0)))
    with pytest.raises(ValueError, match="channel_weights.*2.*Cy = 3"):
        U.compute_loss(ypd, yd, md, True, spec=WeightedLossSpec(channel_weights=(0.5, 1.0)))
    with pytest.raises(ValueError, match="B,T,Cy,H,W"):
        U.compute_loss(ypd.view(6, 3, 8, 8), yd.view(6, 3, 8, 8), None, True, spec=WeightedLossSpec(frame_weights=(0.0, 1.0, 1.0)))
    # a weighted spec without weights is a plain spec: 4-D input is fine
    assert bool(torch.isfinite(U.compute_loss(ypd.view(6, 3, 8, 8), yd.view(6, 3, 8, 8), None, True, spec=WeightedLossSpec(point="l2"))))


def test_the_table_is_built_once_and_kept():
    case = (2, 3, 3, 8, 8)
    ypd, yd, md = on_dev(case, "broadcast")
    spec = WeightedLossSpec(frame_weights=(0.0, 0.375, 1.25), channel_weights=(1.0, 0.7, 2.0))
    U.compute_loss(ypd, yd, md, True, spec=spec)
    q, qsum = ops.plane_weight_table(spec, ypd)
    assert q.dtype == F32 and q.is_cuda and torch.equal(q.cpu(), WC.table(spec, 3, 3)) and qsum == float(WC.table(spec, 3, 3).double().sum())
    n = len(ops._PLANE_W)
    U.compute_loss(ypd, yd, md, True, spec=WeightedLossSpec(frame_weights=[0.0, 0.375, 1.25], channel_weights=[1.0, 0.7, 2.0]))
    assert ops.plane_weight_table(spec, ypd)[0] is q and len(ops._PLANE_W) == n


# ---------------------------------------------------------------------------------------------
# 4. the training step and the graphed step: a tiny model with three output channels
# ---------------------------------------------------------------------------------------------
STEP_SPEC = dict(point="huber", delta=2.0, weight_power=1, weight_gain=0.75, grad_weight=0.02,
                 frame_weights=(0.0, 0.25, 1.5), channel_weights=(1.0, 0.3, 2.0))


def fresh(capturable=False, **opt_kwargs):
    torch.manual_seed(5)
    model = U.TemporalUNetDualView(1, 3, base_ch=8, use_skip_lstm=True).to(DEV).train()
    opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, capturable=capturable, **opt_kwargs)
    d = U.SyntheticSequences(2, 3, 16, 16, seed=6, kind="uniform")
    g = torch.Generator(device="cpu").manual_seed(7)
    y = (torch.rand((2, 3, 3, 16, 16), generator=g) * 2 - 1).to(DEV)
    return model, opt, d.x, y, d.mask


def after_step(loss, opt):
    torch.cuda.synchronize()
    return dict(loss=loss.detach().cpu().clone(), gradients=opt.flat.flat_g.cpu().clone(), parameters=opt.flat.flat_p.cpu().clone())


def test_train_step_with_weights_is_the_step_written_by_hand():
    spec = WeightedLossSpec(**STEP_SPEC)
    with ops.deterministic():
        model, opt, x, y, mask = fresh()
        loss, _ = U.train_step(model, opt, x, y, mask, True, loss=spec)
        a = after_step(loss, opt)
        model, opt, x, y, mask = fresh()
        opt.zero_grad(set_to_none=True)
        y_pred = engine._stack(model(x)[0])
        loss = U.compute_loss(y_pred, y, mask, True, spec=spec)
        loss.backward()
        opt.max_grad_norm = 1.0
        opt.step()
        b = after_step(loss, opt)
        other = float(U.compute_loss(y_pred.detach(), y, mask, True, spec=spec.base))
    assert bool(torch.isfinite(a["loss"])) and float(a["gradients"].abs().max()) > 0
    for key in a:
        assert torch.equal(a[key], b[key]), f"train_step(loss=spec) and the hand-written step differ in {key}"
    want = float(WC.loss_ref(y_pred.detach().cpu(), y.cpu(), mask.cpu(), True, spec))
    assert abs(float(a["loss"]) - want) <= 1e-5 * want and abs(other - want) > 1e-3 * want


def test_fp16_step_with_weights_and_loss_scaling_runs():
    """The scale reaches the kernel through coefs; the loss is computed in f32 from the 16-bit model's prediction, so it is the
    f64 loss of that prediction to the project's f32 tolerance."""
    spec = WeightedLossSpec(**STEP_SPEC)
    with ops.deterministic(), ops.compute_dtype(torch.float16):
        model, opt, x, y, mask = fresh(loss_scale=2.0 ** 14)
        p0 = opt.flat.flat_p.cpu().clone()
        loss, y_pred = U.train_step(model, opt, x, y, mask, True, loss=spec)
        a = after_step(loss, opt)
    assert bool(torch.isfinite(a["loss"])) and bool(torch.isfinite(a["parameters"]).all()) and bool(torch.isfinite(a["gradients"]).all())
    assert not torch.equal(a["parameters"], p0), "the step was skipped: the scaled gradients overflowed"
    want = float(WC.loss_ref(y_pred.float().cpu(), y.cpu(), mask.cpu(), True, spec))
    assert abs(float(a["loss"]) - want) <= 1e-5 * want, (float(a["loss"]), want)


def graph_child():
    """Two eager train_step(loss=weighted spec) from a saved state, then the same two steps as replays of a GraphedTrainStep
    captured with that spec, and a third pair after torch.cuda.empty_cache(), all on one capturable optimiser in deterministic
    mode."""
    spec = WeightedLossSpec(**STEP_SPEC)
    out = {}
    with ops.deterministic():
        model, opt, x, y, mask = fresh(capturable=True)
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        saved = [t.detach().clone() for t in (opt.m, opt.v, opt.hyper)]

        def restore():
            model.load_state_dict(state)
            for t, s in zip((opt.m, opt.v, opt.hyper), saved):
                t.copy_(s)
            ops.weights_changed()

        def two(step):
            res = []
            for _ in range(2):
                loss, _ = step()
                torch.cuda.synchronize()
                res.append([loss.cpu().clone(), opt.flat.flat_p.cpu().clone(), opt.m.cpu().clone(), opt.v.cpu().clone()])
            return res

        eager = two(lambda: U.train_step(model, opt, x, y, mask, True, loss=spec))
        restore()
        g = U.GraphedTrainStep(model, opt, x, y, mask, True, warmup=2, loss=spec)
        out["spec_kept"] = g.loss_spec == spec
        out["table_held"] = g._plane_w is ops.plane_weight_table(spec, g.y_pred)[0]
        restore()
        graphed = two(lambda: g(x, y, mask))
        want = float(WC.loss_ref(g.y_pred.detach().cpu(), y.cpu(), mask.cpu(), True, spec))
        torch.cuda.empty_cache()
        restore()
        again = two(lambda: g(x, y, mask))
    out["finite"] = all(bool(torch.isfinite(t).all()) for step in graphed for t in step)
    out["moved"] = not torch.equal(graphed[0][1], graphed[1][1])
    out["equal"] = {f"{tag} step {i} {what}": bool(torch.equal(a, b)) for tag, runs in (("replay", graphed), ("after empty_cache", again))
                    for i, (e, r) in enumerate(zip(eager, runs))
                    for what, a, b in zip(("loss", "parameters", "exp_avg", "exp_avg_sq"), e, r)}
    out["loss"], out["loss_ref"] = float(graphed[1][0]), want
    return out


def test_graphed_step_with_weights_replays_the_eager_step():
    """In a child process of its own (this file as a script), as the graphed step of tests/test_gpu_loss_spec.py and for its
    reason: one more multi-stream graph in the suite's process."""
    r = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["spec_kept"] and got["table_held"] and got["finite"] and got["moved"], got
    assert all(got["equal"].values()), f"replays and eager steps differ: {[k for k, v in got['equal'].items() if not v]}"
    assert abs(got["loss"] - got["loss_ref"]) <= 1e-5 * got["loss_ref"], got


if __name__ == "__main__":
    print(json.dumps(graph_child()))
