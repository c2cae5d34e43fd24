"""The LossSpec kernels (uclstm_loss_spec_fwd / _fwd_ordered / _bwd) at the C ABI against the f64 restatement of
tests/loss_spec_cases.py, and the loss keyword through compute_loss, train_step, GraphedTrainStep and evaluate.

Bounds (the inputs lie on a 1/64 grid on which rho, rho' and every difference are exact in f32, loss_spec_cases.py):
  * gradient: |grad - ref| <= (weight_power + 6) * 2^-24 * mag, mag = |c1| |rho'| w m + |c2| sum|gradient terms|: `power`
    multiplications and one add for w, three multiplications for the point part, one for c2 * gg, the final add
  * each forward sum (non-negative f32 terms, added in f64): |sum - ref| <= ((weight_power + 4) * 2^-24 + count * 2^-52) * ref
  * compute_loss: with e the forward bound, the two quotients and the rounding of the loss to f32 give
    |loss - ref| <= (2 e / (1 - e) + 2^-24 + 2^-50) * ref; the coefficients the backward kernel reads are the f32 roundings of
    quotients of those sums, off by at most dc = e / (1 - e) + 2 * 2^-24 relatively, so
    |grad - ref| <= ((weight_power + 6) * 2^-24 * (1 + dc) + dc) * mag
Outputs are pre-filled with NaN and every element is compared.
"""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_cases as BC
import loss_spec_cases as LC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import engine, ops
    from unet_convlstm_amd.loss import LossSpec

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
F32_UNIT = LC.F32_UNIT


def p_(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    L.check(getattr(L.lib, name)(*args, ops._stream()), name)


def nan_dev(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def on_dev(case, masked):
    yp, y, mask = LC.inputs(case, masked)
    return yp.to(DEV), y.to(DEV), (mask.to(DEV) if masked else None)


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
        bound = LC.fwd_rel_bound(spec, counts[k]) * float(ref[k])
        err = abs(float(got[k]) - float(ref[k]))
        print(f"[parity] {what} sums[{k}]: |err| {err:.3e}, bound {bound:.3e}, value {float(ref[k]):.6e}")
        assert err <= bound, f"{what}: sums[{k}] = {float(got[k])!r}, f64 {float(ref[k])!r}, |err| {err:.3e} > {bound:.3e}"
    if spec.grad_weight == 0:
        assert float(got[2]) == 0.0 and float(got[3]) == 0.0, f"{what}: gradient sums {got[2:].tolist()} without a gradient term"


def label(name, case, masked):
    width = "V4" if LC.vectorised(LC.SPECS[name], case) else "V1"
    return f"{name} {case} {'masked' if masked else 'mask NULL'} ({width})"


# ---------------------------------------------------------------------------------------------
# 1. C ABI
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,masked", LC.runs(), ids=str)
def test_spec_bwd_against_f64(name, case, masked):
    spec, (planes, H, W) = LC.SPECS[name], case
    yp, y, mask = LC.inputs(case, masked)
    ypd, yd, md = on_dev(case, masked)
    desc = ops.loss_spec_desc(spec)
    cd = torch.tensor(BC.LOSS_COEFS, dtype=F32, device=DEV)
    grad = nan_dev((planes, H, W), F32)
    call("uclstm_loss_spec_bwd", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(cd), p_(grad), planes, H, W)
    c1, c2 = (float(v) for v in cd.cpu().double())
    ref, mag = LC.loss_bwd_ref(yp, y, mask, spec, c1, c2)
    check_bound(grad, ref, LC.n_bwd(spec) * F32_UNIT * mag, f"loss_spec_bwd {label(name, case, masked)}")


@pytest.mark.parametrize("name,case,masked", LC.runs(), ids=str)
def test_spec_fwd_sums_against_f64(name, case, masked):
    spec, (planes, H, W) = LC.SPECS[name], case
    yp, y, mask = LC.inputs(case, masked)
    ypd, yd, md = on_dev(case, masked)
    desc = ops.loss_spec_desc(spec)
    ref, counts = LC.sums_ref(yp, y, mask, spec)
    sums = torch.zeros(4, dtype=F64, device=DEV)
    call("uclstm_loss_spec_fwd", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(sums), planes, H, W)
    check_sums(sums, ref, counts, spec, f"loss_spec_fwd {label(name, case, masked)}")
    if name == "reference":                # the reference's own kernel meets the same bound against the same f64 sums
        legacy = torch.zeros(4, dtype=F64, device=DEV)
        call("uclstm_loss_fwd", p_(ypd), p_(yd), p_(md), p_(legacy), planes, H, W)
        check_sums(legacy, ref, counts, spec, f"loss_fwd {case} {'masked' if masked else 'mask NULL'}")


def ordered_sum(partials, start=None):
    """out = start (or 0) + partials[0] + partials[1] + ... left to right in f64, one rounding per addition."""
    acc = np.zeros(partials.shape[1], dtype=np.float64) if start is None else start.astype(np.float64).copy()
    for r in range(partials.shape[0]):
        acc = acc + partials[r]
    return acc


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("case", LC.CASES, ids=str)
@pytest.mark.parametrize("name", LC.LARGE_SPECS, ids=str)
def test_spec_fwd_ordered_finishes_in_row_order(name, case, masked):
    spec, (planes, H, W) = LC.SPECS[name], case
    yp, y, mask = LC.inputs(case, masked)
    ypd, yd, md = on_dev(case, masked)
    desc = ops.loss_spec_desc(spec)
    rows = int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W))
    assert rows == min(1024, (planes * H * W + 255) // 256)
    ref, counts = LC.sums_ref(yp, y, mask, spec)
    base = torch.tensor([0.5, 1.5, 2.5, 3.5], dtype=F64)
    what = f"loss_spec_fwd_ordered {label(name, case, masked)} ({rows} rows)"
    for accumulate in (0, 1):
        bits = []
        for _ in range(2):
            partials, sums = nan_dev((rows, 4), F64), (base.to(DEV) if accumulate else nan_dev((4,), F64))
            call("uclstm_loss_spec_fwd_ordered", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(partials), p_(sums), accumulate, planes, H, W)
            prt, got = partials.cpu().numpy(), sums.cpu().numpy()
            assert np.isfinite(prt).all() and np.isfinite(got).all(), f"{what}: partial rows or sums not written"
            want = ordered_sum(prt, base.numpy() if accumulate else None)
            assert got.tobytes() == want.tobytes(), f"{what} accumulate={accumulate}: {got} is not the in-order sum {want}"
            bits.append(prt.tobytes() + got.tobytes())
        assert bits[0] == bits[1], f"{what} accumulate={accumulate}: two launches differ"
        if not accumulate:
            check_sums(torch.from_numpy(got), ref, counts, spec, what)


# ---------------------------------------------------------------------------------------------
# 2. compute_loss(spec=...)
# ---------------------------------------------------------------------------------------------
HOST_SPECS = ("reference", "masked_mse", "l2_refweight", "huber2_p1", "huber_nograd")
HOST_CASES = [((5, 17, 19), (5, 1, 1, 17, 19)), ((3, 8, 8), (1, 3, 1, 8, 8))]
MODES = [("masked", True, True), ("use_mask=False", True, False), ("mask=None", False, True)]


def run_loss(yp, y, mask, use_mask, spec, forced=False):
    """loss and d loss / d y_pred on the device; forced: straight into ops.LossFn, past compute_loss's reference detection."""
    leaf = yp.clone().requires_grad_(True)
    loss = ops.LossFn.apply(leaf, y, mask, use_mask, spec) if forced else U.compute_loss(leaf, y, mask, use_mask, spec=spec)
    loss.backward()
    return loss.detach(), leaf.grad


@pytest.mark.parametrize("mode,with_mask,use_mask", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("case,shape", HOST_CASES, ids=str)
@pytest.mark.parametrize("name", HOST_SPECS, ids=str)
@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "ordered"])
def test_compute_loss_with_a_spec_against_f64(deterministic, name, case, shape, mode, with_mask, use_mask):
    spec = LC.SPECS[name]
    yp, y, mask = LC.inputs(case, with_mask)
    ypd, yd, md = (t.to(DEV).view(shape) if t is not None else None for t in (yp, y, mask))
    ops.LAUNCH_LOG = []
    try:
        with ops.deterministic(deterministic):
            loss, grad = run_loss(ypd, yd, md, use_mask, spec, forced=(name == "reference"))
        log = list(ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
    assert log == [("reduce", "loss_fwd_ordered" if deterministic else "loss_fwd")]
    masked = with_mask and use_mask
    m_eff = mask if masked else None
    want = float(LC.loss_ref(yp, y, mask, use_mask, spec))
    e = LC.fwd_rel_bound(spec, yp.numel())
    tol = (2 * e / (1 - e) + F32_UNIT + 2.0 ** -50) * want
    what = f"compute_loss {name} {case} {mode} {'ordered' if deterministic else 'atomic'}"
    print(f"[parity] {what}: loss {float(loss)!r}, f64 {want!r}, |err| {abs(float(loss) - want):.3e}, bound {tol:.3e}")
    assert loss.dtype == F32 and abs(float(loss) - want) <= tol, what
    c1, c2 = LC.coefs_ref(y, m_eff, masked, spec)
    ref, mag = LC.loss_bwd_ref(yp, y, m_eff, spec, c1, c2)
    dc = e / (1 - e) + 2 * F32_UNIT
    check_bound(grad.view(yp.shape), ref, (LC.n_bwd(spec) * F32_UNIT * (1 + dc) + dc) * mag, f"{what} gradient")


@pytest.mark.parametrize("shape", [(2, 3, 1, 7, 1), (2, 3, 1, 1, 7)], ids=str)
def test_a_plane_without_cells_has_a_finite_loss_without_the_gradient_term(shape):
    torch.manual_seed(3)
    yp, y = torch.randn(shape), torch.randn(shape)
    mask = (torch.rand(shape) > 0.3).float()
    for spec in (LossSpec.masked_mse(), LC.SPECS["l1_nograd"], LC.SPECS["huber_nograd"]):
        for m, use_mask in ((mask, True), (mask, False), (None, True)):
            loss, grad = run_loss(yp.to(DEV), y.to(DEV), None if m is None else m.to(DEV), use_mask, spec)
            want = float(LC.loss_ref(yp, y, m, use_mask, spec))
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and want > 0
            assert abs(float(loss) - want) <= 1e-5 * want, (spec, use_mask, float(loss), want)          # the project's f32 tolerance
    # the gradient term of the reference on the same planes: the empty mean, as main.py:68
    assert bool(torch.isnan(U.compute_loss(yp.to(DEV), y.to(DEV), None, False)))


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "ordered"])
def test_the_default_spec_takes_the_reference_kernels(deterministic):
    """spec=None, LossSpec() and LossSpec.reference() are one path: equal bits and the same launch log.  Atomic form on one block
    (192 elements: one addition per sum, so its bits do not depend on an order); ordered form on seven blocks."""
    case, shape = ((5, 17, 19), (5, 1, 1, 17, 19)) if deterministic else ((3, 8, 8), (1, 3, 1, 8, 8))
    yp, y, mask = (t.to(DEV).view(shape) for t in LC.inputs(case, True))
    got = []
    for spec in (None, LossSpec(), LossSpec.reference()):
        ops.LAUNCH_LOG = []
        try:
            with ops.deterministic(deterministic):
                loss, grad = run_loss(yp, y, mask, True, spec)
            got.append((loss.cpu(), grad.cpu(), list(ops.LAUNCH_LOG)))
        finally:
            ops.LAUNCH_LOG = None
    assert got[0][2] == [("reduce", "loss_fwd_ordered" if deterministic else "loss_fwd")]
    for loss, grad, log in got[1:]:
        assert torch.equal(loss, got[0][0]) and torch.equal(grad, got[0][1]) and log == got[0][2]


# ---------------------------------------------------------------------------------------------
# 3. the training step, the graphed step, evaluation
# ---------------------------------------------------------------------------------------------
def fresh(capturable=False, **opt_kwargs):
    torch.manual_seed(5)
    model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV).train()
    opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, capturable=capturable, **opt_kwargs)
    return model, opt, U.SyntheticSequences(2, 3, 32, 32, seed=6, kind="uniform")


def after_step(loss, opt):
    torch.cuda.synchronize()
    return dict(loss=loss.detach().cpu().clone(), gradients=opt.flat.flat_g.cpu().clone(), parameters=opt.flat.flat_p.cpu().clone())


@pytest.mark.parametrize("name", ["masked_mse", "huber2_p1"], ids=str)
def test_train_step_with_a_spec_is_the_step_written_by_hand(name):
    spec = LC.SPECS[name]
    with ops.deterministic():
        model, opt, d = fresh()
        loss, _ = U.train_step(model, opt, d.x, d.y, d.mask, True, loss=spec)
        a = after_step(loss, opt)
        model, opt, d = fresh()
        opt.zero_grad(set_to_none=True)
        y_pred = engine._stack(model(d.x)[0])
        loss = U.compute_loss(y_pred, d.y, d.mask, True, spec=spec)
        loss.backward()
        opt.max_grad_norm = 1.0
        opt.step()
        b = after_step(loss, opt)
        # and it is this spec's loss that ran: the reference's loss of the same prediction is another number
        other = float(U.compute_loss(y_pred.detach(), d.y, d.mask, True))
    assert bool(torch.isfinite(a["loss"])) and float(a["gradients"].abs().max()) > 0
    for key in a:
        assert torch.equal(a[key], b[key]), f"{name}: train_step(loss=spec) and the hand-written step differ in {key}"
    want = float(LC.loss_ref(y_pred.detach().cpu(), d.y.cpu(), d.mask.cpu(), True, spec))
    assert abs(float(a["loss"]) - want) <= 1e-5 * want and abs(other - want) > 1e-3 * want


def test_fp16_step_with_a_spec_and_loss_scaling_runs():
    with ops.deterministic(), ops.compute_dtype(torch.float16):
        model, opt, d = fresh(loss_scale=2.0 ** 14)
        p0 = opt.flat.flat_p.cpu().clone()
        loss, _ = U.train_step(model, opt, d.x, d.y, d.mask, True, loss=LossSpec.masked_mse())
        a = after_step(loss, opt)
    assert bool(torch.isfinite(a["loss"])) and bool(torch.isfinite(a["parameters"]).all()) and bool(torch.isfinite(a["gradients"]).all())
    assert not torch.equal(a["parameters"], p0), "the step was skipped: the scaled gradients overflowed"


def graph_child():
    """Two eager train_step(loss=masked_mse) from a saved state, then the same two steps as replays of a GraphedTrainStep captured
    with that spec, both on one capturable optimiser, in deterministic mode."""
    spec = LossSpec.masked_mse()
    out = {}
    with ops.deterministic():
        model, opt, d = fresh(capturable=True)
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

        eager = two(lambda: U.train_step(model, opt, d.x, d.y, d.mask, True, loss=spec))
        restore()
        g = U.GraphedTrainStep(model, opt, d.x, d.y, d.mask, True, warmup=2, loss=spec)
        out["spec_kept"] = g.loss_spec == spec
        restore()
        graphed = two(lambda: g(d.x, d.y, d.mask))
    out["finite"] = all(bool(torch.isfinite(t).all()) for step in graphed for t in step)
    out["moved"] = not torch.equal(graphed[0][1], graphed[1][1])
    out["equal"] = {f"step {i} {what}": bool(torch.equal(a, b)) for i, (e, r) in enumerate(zip(eager, graphed))
                    for what, a, b in zip(("loss", "parameters", "exp_avg", "exp_avg_sq"), e, r)}
    want = float(LC.loss_ref(g.y_pred.detach().cpu(), d.y.cpu(), d.mask.cpu(), True, spec))
    out["loss"], out["loss_ref"] = float(graphed[1][0]), want
    return out


def test_graphed_step_with_a_spec_replays_the_eager_step():
    """In a child process of its own (this file as a script), as the graphed step of tests/test_gpu_deterministic.py and for its
    reason: a third multi-stream graph in the suite's process."""
    r = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["spec_kept"] and got["finite"] and got["moved"], got
    assert all(got["equal"].values()), f"replays and eager steps differ: {[k for k, v in got['equal'].items() if not v]}"
    assert abs(got["loss"] - got["loss_ref"]) <= 1e-5 * got["loss_ref"], got


def test_evaluate_returns_the_loss_of_the_spec(tmp_path):
    rng = np.random.default_rng(0)
    N, T, H, W = 4, 3, 32, 32
    X = (rng.random((N, T, 2, H, W)) * 30).astype(np.float32)
    X[X < 6] = 0.0
    Y = np.tanh(X[:, :, :1] / 15.0 - 1.0).astype(np.float32) * 4.0
    path = tmp_path / "eval.npz"
    np.savez(path, X=X, Y=Y)
    ds = U.NPZSequenceDataset(str(path))
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False)
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV)
    spec, dev = LC.SPECS["huber2_p1"], torch.device(DEV)
    with ops.deterministic():
        got = U.evaluate(model, loader, dev, ds, use_mask=True, loss=spec)
        rep = U.evaluate_report(model, loader, dev, ds, use_mask=True, loss=spec)
        plain = U.evaluate(model, loader, dev, ds, use_mask=True)
        want, n = 0.0, 0
        with torch.no_grad():
            for x, y, mask in loader:
                y_pred = engine._stack(model(x.to(DEV))[0]).cpu()
                want += float(LC.loss_ref(y_pred, y, mask, True, spec)) * x.size(0)
                n += x.size(0)
    want /= n
    assert np.isfinite(got[0]) and abs(got[0] - want) <= 1e-5 * want, (got[0], want)
    assert got[0] == rep[0] and got[1:] == plain[1:] and abs(plain[0] - want) > 1e-3 * want


if __name__ == "__main__":
    print(json.dumps(graph_child()))
