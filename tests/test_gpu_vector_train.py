"""GPU tests of the vector-target path around the model: the loss with a channel-broadcast mask (uclstm_loss_spec_*_bc) against
the LossSpec kernels fed the expanded mask and against f64, the per-channel metric sums (uclstm_metric_sums_vec), and the whole
path end to end: VectorNPZDataset -> DeviceSequenceLoader(augment) -> a model with three outputs -> train_step -> evaluate(tta)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import loss_spec_cases as LC
import vector_cases as VC
from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import engine, ops

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
F32_UNIT = LC.F32_UNIT
CY = 3
# (frames, H, W): planes = frames * CY.  5 x 7 and 12 x 12 as the issue names them; 4 frames of 5 x 7 make the whole array a
# multiple of four long while a plane is not (the 16-byte instances with a group of four across two planes), 3 frames do not.
BC_CASES = [(3, 5, 7), (4, 5, 7), (2, 12, 12)]
BC_SPECS = ("reference", "masked_mse", "l2_refweight", "huber2_p1", "huber_nograd", "l1_nograd")


def p_(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    L.check(getattr(L.lib, name)(*args, ops._stream()), name)


def nan_dev(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


_inputs = {}


def bc_inputs(case):
    """y_pred, y [frames * CY, H, W] on the 1/64 grid of loss_spec_cases, the one-channel mask [frames, H, W] and its expansion
    [frames * CY, H, W]; drawn once, read-only."""
    if case not in _inputs:
        frames, H, W = case
        yp, y, _ = LC.inputs((frames * CY, H, W), False)
        mask = LC.inputs((frames, H, W), True)[2]
        _inputs[case] = (yp, y, mask, mask.repeat_interleave(CY, dim=0).contiguous())
    return _inputs[case]


@pytest.mark.parametrize("case", BC_CASES, ids=str)
@pytest.mark.parametrize("name", BC_SPECS, ids=str)
def test_bc_kernels_equal_the_spec_kernels_on_the_expanded_mask(name, case):
    spec, (frames, H, W) = LC.SPECS[name], case
    planes = frames * CY
    yp, y, mask, full = bc_inputs(case)
    ypd, yd, md, fd = (t.to(DEV) for t in (yp, y, mask, full))
    desc = ops.loss_spec_desc(spec)
    # bwd: bit-identical
    cd = torch.tensor([0.37, 0.011], dtype=F32, device=DEV)
    g_bc, g_full = nan_dev((planes, H, W), F32), nan_dev((planes, H, W), F32)
    call("uclstm_loss_spec_bwd_bc", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(cd), p_(g_bc), planes, H, W, CY)
    call("uclstm_loss_spec_bwd", C.byref(desc), p_(ypd), p_(yd), p_(fd), p_(cd), p_(g_full), planes, H, W)
    assert bool(torch.isfinite(g_bc).all()) and torch.equal(g_bc, g_full), f"bwd {name} {case}: {int((g_bc != g_full).sum())} elements differ"
    # ordered fwd: the same partial rows and the same sums, bit for bit
    rows = int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W))
    out = []
    for entry, m, extra in (("uclstm_loss_spec_fwd_ordered_bc", md, (CY,)), ("uclstm_loss_spec_fwd_ordered", fd, ())):
        partials, sums = nan_dev((rows, 4), F64), nan_dev((4,), F64)
        call(entry, C.byref(desc), p_(ypd), p_(yd), p_(m), p_(partials), p_(sums), 0, planes, H, W, *extra)
        out.append((partials.cpu(), sums.cpu()))
    assert bool(torch.isfinite(out[0][0]).all()) and torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), (name, case)
    # atomic fwd: against f64 within the bound of the LossSpec tests
    ref, counts = LC.sums_ref(yp, y, full, spec)
    sums = torch.zeros(4, dtype=F64, device=DEV)
    call("uclstm_loss_spec_fwd_bc", C.byref(desc), p_(ypd), p_(yd), p_(md), p_(sums), planes, H, W, CY)
    got = sums.cpu()
    for k in range(4):
        bound = LC.fwd_rel_bound(spec, counts[k]) * float(ref[k])
        err = abs(float(got[k]) - float(ref[k]))
        print(f"[parity] loss_spec_fwd_bc {name} {case} sums[{k}]: |err| {err:.3e}, bound {bound:.3e}, value {float(ref[k]):.6e}")
        assert err <= bound, (name, case, k, float(got[k]), float(ref[k]))
    assert float(ref[1]) != float(LC.sums_ref(yp, y, None, spec)[0][1])          # the mask matters


MODES = [("masked", True), ("use_mask=False", False)]


@pytest.mark.parametrize("mode,use_mask", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("case", [(4, 5, 7), (2, 12, 12)], ids=str)
@pytest.mark.parametrize("name", ("reference", "masked_mse", "huber2_p1", "huber_nograd"), ids=str)
@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "ordered"])
def test_compute_loss_broadcasts_a_one_channel_mask(deterministic, name, case, mode, use_mask):
    """y [B,T,3,H,W] with mask [B,T,1,H,W] through compute_loss and .backward(), against loss_ref / loss_bwd_ref on the expanded mask
    with the bounds of tests/test_gpu_loss_spec.py.  spec=None (the reference's loss) takes the same path as LossSpec.reference()."""
    spec, (frames, H, W) = LC.SPECS[name], case
    yp, y, mask, full = bc_inputs(case)
    shape, mshape = (1, frames, CY, H, W), (1, frames, 1, H, W)
    ypd, yd, md = yp.to(DEV).view(shape), y.to(DEV).view(shape), mask.to(DEV).view(mshape)
    calls = []
    names = [n for n in L._PROTOS if n.startswith("uclstm_loss_")]
    saved = {n: getattr(L.lib, n) for n in names}
    try:
        for n in names:
            setattr(L.lib, n, (lambda f, k: lambda *a: (calls.append(k), f(*a))[1])(saved[n], n))
        with ops.deterministic(deterministic):
            leaf = ypd.clone().requires_grad_(True)
            loss = U.compute_loss(leaf, yd, md, use_mask, spec=None if name == "reference" else spec)
            loss.backward()
            loss = loss.detach()
    finally:
        for n in names:
            setattr(L.lib, n, saved[n])
    if use_mask:
        assert calls == ["uclstm_loss_fwd_ordered_rows", "uclstm_loss_spec_fwd_ordered_bc", "uclstm_loss_spec_bwd_bc"] if deterministic else \
            calls == ["uclstm_loss_spec_fwd_bc", "uclstm_loss_spec_bwd_bc"], calls
    else:
        assert not any(n.endswith("_bc") for n in calls), calls              # no mask: the entry points of today
    m_eff = full if use_mask else None
    want = float(LC.loss_ref(yp, y, full, use_mask, spec))
    e = LC.fwd_rel_bound(spec, yp.numel())
    tol = (2 * e / (1 - e) + F32_UNIT + 2.0 ** -50) * want
    what = f"compute_loss bc {name} {case} {mode} {'ordered' if deterministic else 'atomic'}"
    print(f"[parity] {what}: loss {float(loss)!r}, f64 {want!r}, |err| {abs(float(loss) - want):.3e}, bound {tol:.3e}")
    assert loss.dtype == F32 and abs(float(loss) - want) <= tol, what
    c1, c2 = LC.coefs_ref(y, m_eff, use_mask, spec)
    ref, mag = LC.loss_bwd_ref(yp, y, m_eff, spec, c1, c2)
    dc = e / (1 - e) + 2 * F32_UNIT
    bound = (LC.n_bwd(spec) * F32_UNIT * (1 + dc) + dc) * mag
    d = (leaf.grad.view(yp.shape).double().cpu() - ref).abs()
    assert bool(torch.isfinite(leaf.grad).all()) and int((d > bound).sum()) == 0, f"{what} gradient: worst {float((d / (bound + 1e-300)).max()):.3f} x"


def test_a_mask_with_all_channels_keeps_the_entry_points_of_today():
    yp, y, mask, full = bc_inputs((2, 12, 12))
    shape = (1, 2, CY, 12, 12)
    calls = []
    names = [n for n in L._PROTOS if n.startswith("uclstm_loss_")]
    saved = {n: getattr(L.lib, n) for n in names}
    try:
        for n in names:
            setattr(L.lib, n, (lambda f, k: lambda *a: (calls.append(k), f(*a))[1])(saved[n], n))
        leaf = yp.to(DEV).view(shape).clone().requires_grad_(True)
        a = U.compute_loss(leaf, y.to(DEV).view(shape), full.to(DEV).view(shape), True)
        a.backward()
        U.compute_loss(leaf.detach(), y.to(DEV).view(shape), full.to(DEV).view(shape), True, spec=LC.SPECS["masked_mse"])
    finally:
        for n in names:
            setattr(L.lib, n, saved[n])
    assert calls == ["uclstm_loss_fwd", "uclstm_loss_bwd", "uclstm_loss_spec_fwd"], calls
    b = U.compute_loss(yp.to(DEV).view(shape), y.to(DEV).view(shape), mask.to(DEV).view(1, 2, 1, 12, 12), True)
    assert abs(float(a) - float(b)) <= 1e-6 * abs(float(a))                  # the broadcast IS the expanded mask


# ---------------------------------------------------------------------------------------------
# metrics per component
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vec_ds(tmp_path_factory):
    root = tmp_path_factory.mktemp("vector_train")
    out = {}
    for transform in ("asinh", "signed_log", None):
        VC.write_npz(root / "m.npz", 4, 2, 2, CY, 12, 12, seed=3)
        out[transform] = U.VectorNPZDataset(str(root / "m.npz"), VC.AXES_UVW, tie_horizontal=True, lower_percentile=1.0,
                                            upper_percentile=99.0, y_transform=transform)
    return out


def _metric_call(consts, transform, yp, y, mask, sums, accumulate):
    Cy, (H, W) = yp.shape[-3], yp.shape[-2:]
    n_frames = yp.numel() // (Cy * H * W)
    rows = int(L.lib.uclstm_metric_sums_vec_rows(n_frames, Cy, H * W))
    assert rows == min(1024, (n_frames * H * W + 255) // 256)
    partials = nan_dev((rows, Cy, 4), F64)
    call("uclstm_metric_sums_vec", p_(yp), p_(y), p_(mask), p_(partials), p_(sums), accumulate, n_frames, Cy, H * W,
         engine._TRANSFORM_IDS[transform], consts)
    return partials


def _close(got, ref, what):
    """Relative 1e-5 as tests/test_gpu_data.py::test_metric_sums_match_main_py_formulas: the sums of |d|, d^2 and the count relative to
    themselves (floored at the count, i.e. a mean of 1), the signed sum absolutely, 1e-5 per counted pixel."""
    got, ref = got.double().cpu(), ref.double().cpu()
    for c in range(ref.shape[0]):
        a, q, e, n = (float(v) for v in ref[c])
        for k, scale in ((0, max(a, n)), (1, max(q, n)), (2, n), (3, n)):
            err = abs(float(got[c, k]) - float(ref[c, k]))
            print(f"[metric] {what} channel {c} sums[{k}]: |err| {err:.3e}, bound {1e-5 * scale:.3e}")
            assert err <= 1e-5 * scale, (what, c, k, float(got[c, k]), float(ref[c, k]))
        assert float(got[c, 3]) == n


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("transform", ["asinh", "signed_log", None], ids=str)
@pytest.mark.parametrize("shape", [(2, 3, CY, 12, 12), (1, 5, CY, 5, 7)], ids=str)
def test_metric_sums_vec_against_f64_per_channel(vec_ds, shape, transform, masked):
    ds = vec_ds[transform]
    torch.manual_seed(shape[-1])
    y = torch.rand(shape) * 2 - 1
    yp = y + 0.1 * torch.randn(shape)
    mask = (torch.rand(shape[:2] + (1,) + shape[3:]) > 0.4).float() if masked else None
    ref = VC.metric_sums64(yp, y, mask, ds)
    ypd, yd, md = yp.to(DEV), y.to(DEV), (mask.to(DEV) if masked else None)
    sums = nan_dev((CY, 4), F64)
    p1 = _metric_call(ds.target_consts(), transform, ypd, yd, md, sums, 0)
    first = sums.cpu().clone()
    _close(first, ref, f"{shape} {transform} masked={masked}")
    assert len({float(ref[c, 0]) for c in range(CY)}) == CY                 # per-channel constants give per-channel sums
    # two calls give identical bits; accumulate adds to the earlier sums
    sums2 = nan_dev((CY, 4), F64)
    p2 = _metric_call(ds.target_consts(), transform, ypd, yd, md, sums2, 0)
    assert torch.equal(p1, p2) and torch.equal(sums2.cpu(), first) and bool(torch.isfinite(p1).all())
    _metric_call(ds.target_consts(), transform, ypd, yd, md, sums2, 1)
    acc = first.clone()
    for r in range(p1.shape[0]):
        acc = acc + p1[r].cpu()
    assert torch.equal(sums2.cpu(), acc)


def test_metric_sums_vec_with_one_channel_agrees_with_the_ordered_scalar_kernel(vec_ds):
    ds = vec_ds["asinh"]
    torch.manual_seed(1)
    y = (torch.rand(2, 3, 1, 12, 12) * 2 - 1).to(DEV)
    yp = y + 0.1 * torch.randn_like(y)
    mask = (torch.rand_like(y) > 0.4).float()
    one = (L.TargetConsts * 1)(ds.target_consts()[2])
    sums = nan_dev((1, 4), F64)
    _metric_call(one, "asinh", yp, y, mask, sums, 0)
    n = y.numel()
    partials, old = nan_dev((int(L.lib.uclstm_metric_sums_ordered_rows(n)), 4), F64), nan_dev((4,), F64)
    call("uclstm_metric_sums_ordered", p_(yp), p_(y), p_(mask), p_(partials), p_(old), 0, n, float(ds.y_scale[2]), float(ds.trans_min[2]),
         float(ds.trans_max[2]))
    _close(sums, old.view(1, 4), "Cy = 1 against metric_sums_ordered")


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def _wind_npz(path, N, T, S, seed):
    rng = np.random.default_rng(seed)
    X = (rng.random((N, T, 2, S, S)) * 30).astype(np.float32)
    X[X < 6] = 0.0
    base = np.tanh(X[:, :, :1] / 15.0 - 1.0).astype(np.float32)
    Y = np.concatenate([base * 9.0 + rng.standard_normal(base.shape).astype(np.float32), np.roll(base, 3, axis=-1) * -8.0,
                        base * 1.5], axis=2).astype(np.float32)
    np.savez(path, X=X, Y=Y)


def _run_end_to_end(tmp_path, model, S, steps, B=2, T=3):
    _wind_npz(tmp_path / "wind.npz", 4, T, S, seed=S)
    ds = U.VectorNPZDataset(str(tmp_path / "wind.npz"), VC.AXES_UVW, tie_horizontal=True, lower_percentile=0.5, upper_percentile=99.5)
    loader = U.DeviceSequenceLoader(ds, B, augment=U.Augment(hflip=True, vflip=True, transpose=True),
                                    augment_generator=torch.Generator().manual_seed(S))
    opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    model.train()
    losses, first = [], None
    it = iter(loader)
    for k in range(steps):
        try:
            x, y, mask = next(it)
        except StopIteration:
            it = iter(loader)
            x, y, mask = next(it)
        assert tuple(y.shape) == (B, T, 3, S, S) and tuple(mask.shape) == (B, T, 1, S, S)
        loss, y_pred = U.train_step(model, opt, x, y, mask, True)
        if first is None:
            first = (float(loss), y_pred.float().cpu(), y.cpu(), mask.cpu())
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses), losses
    # the first loss against the f64 oracle loss of that batch (the reference's loss, the mask broadcast over the channels)
    got, y_pred, y, mask = first
    spec = LC.SPECS["reference"]
    want = float(LC.loss_ref(y_pred, y, mask.expand_as(y), True, spec))
    e = LC.fwd_rel_bound(spec, y.numel())
    tol = (2 * e / (1 - e) + F32_UNIT + 2.0 ** -50) * want
    print(f"[end to end] first loss {got!r}, f64 {want!r}, |err| {abs(got - want):.3e}, bound {tol:.3e}; losses {losses}")
    assert abs(got - want) <= tol
    return ds, opt


def test_end_to_end_with_the_dual_view_model(tmp_path):
    base_ch = int(load_golden("model_skip")["p/inc.net.0.weight"].shape[0])      # the width of the golden-model tests
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 3, base_ch=base_ch, lstm_layers=1, use_skip_lstm=True).to(DEV)
    ds, opt = _run_end_to_end(tmp_path, model, 32, steps=3)
    dev = torch.device(DEV)
    plain = U.DeviceSequenceLoader(ds, 2)
    out = U.evaluate(model, plain, dev, ds, use_mask=True, tta="d4", per_channel=True)
    assert len(out) == 5 and all(math.isfinite(v) for v in out[:4])
    per = out[4]
    assert sorted(per) == ["mae", "me", "rmse"] and all(len(per[k]) == 3 for k in per)
    # the same predictions in torch f64
    model.eval()
    sums = torch.zeros(3, 4, dtype=F64)
    with torch.no_grad():
        for x, y, mask in plain:
            y_pred = U.predict_tta(model, x, "d4", dataset=ds)
            sums += VC.metric_sums64(y_pred.cpu(), y.cpu(), mask.cpu(), ds)
    for c in range(3):
        a, q, e, n = (float(v) for v in sums[c])
        assert abs(per["mae"][c] - a / n) <= 1e-5 * (a / n), (c, per["mae"][c], a / n)
        assert abs(per["rmse"][c] - math.sqrt(q / n)) <= 1e-5 * math.sqrt(q / n)
    a, q, e, n = (float(v) for v in sums.sum(dim=0))
    assert abs(out[1] - a / n) <= 1e-5 * (a / n) and abs(out[2] - math.sqrt(q / n)) <= 1e-5 * math.sqrt(q / n)      # pooled
    assert len(U.evaluate(model, plain, dev, ds, use_mask=True)) == 4
    tr = U.train_one_epoch(model, plain, opt, dev, ds, use_mask=True, per_channel=True)
    assert len(tr) == 5 and len(tr[4]["mae"]) == 3 and all(math.isfinite(v) for v in tr[:4])


def test_one_step_with_the_resnet_model(tmp_path):
    torch.manual_seed(0)
    model = U.PretrainedTemporalUNet(out_channels=3).to(DEV)
    _run_end_to_end(tmp_path, model, 64, steps=1)
