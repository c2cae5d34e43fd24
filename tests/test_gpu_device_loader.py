"""GPU tests of the device-resident loader: uclstm_dataset_gather_transform against NPZSequenceDataset.__getitem__ (three target
transforms, clip on / off, vector and scalar paths, every kind of index vector), DeviceSequenceLoader against a DataLoader over
the same sampler, the shared device copy, static output buffers, and the epoch loops of main.py fed from the device."""
import math

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, RandomSampler, random_split

from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import engine as E

DEV = "cuda"
X_TOL = dict(rtol=1e-6, atol=1e-7)          # tests/test_gpu_data.py
Y_TOL = dict(rtol=1e-5, atol=2e-6)          # tests/test_gpu_data.py (asinh)
TRANSFORMS = ["asinh", "signed_log", None]


# ---------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------
def _edges(X, Y):
    """Plant the values at which the arithmetic can go wrong: targets outside [min_y, max_y] (defaults -7.60 / 8.78), exact
    zeros of both signs, raw channel-0 values at float32(1.1) and its two neighbours."""
    t = np.float32(1.1)
    first, last, y = X[0, 0, 0].reshape(-1), X[-1, -1, 0].reshape(-1), Y.reshape(-1)          # views
    first[:3] = [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(2))]
    last[-3:] = first[:3]                                                  # ... and in the last frame's last pixels
    y[:6] = [-20.0, 15.0, 0.0, -0.0, -7.6, 8.79]
    y[-4:] = [0.0, 40.0, -30.0, 1e-30]
    return X, Y


def _raw(case):
    if case.startswith("golden"):                                          # N = 3, T = 4, C = 2, 8 x 8: 16-byte path, C = 2
        g = load_golden("dataset")
        X, Y = g["X"].numpy().copy(), g["Y"].numpy().copy()
        return _edges(X, Y) if case == "golden+edges" else (X, Y)
    rng = np.random.default_rng(len(case))
    N, T, C, H, W = {"5x7": (5, 1, 2, 5, 7), "c4": (4, 3, 4, 4, 8)}[case]  # HW = 35: scalar path; C = 4: run-time channel loop
    X = (rng.random((N, T, C, H, W)) * 40).astype(np.float32)
    X[X < 8] = 0.0
    Y = (rng.standard_normal((N, T, 1, H, W)) * 3).astype(np.float32)
    return _edges(X, Y)


CASES = ["golden", "golden+edges", "5x7", "c4"]
_cache = {}


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(case, transform, clip) -> (dataset, host rows [(x, y, mask)], x_all, y_all on the device); built once, never changed."""
    root = tmp_path_factory.mktemp("device_loader")

    def get(case, transform, clip):
        key = (case, transform, clip)
        if key not in _cache:
            path = root / f"{case}.npz"
            if not path.exists():
                X, Y = _raw(case)
                np.savez(path, X=X, Y=Y)
            ds = U.NPZSequenceDataset(str(path), y_transform=transform, clip_outliers=clip)
            host = [ds[i] for i in range(len(ds))]
            _cache[key] = (ds, host, torch.from_numpy(ds.X).to(DEV), torch.from_numpy(ds.Y).to(DEV))
        return _cache[key]
    return get


def _y64(ds, rows):
    """train/unet.py:287-299 evaluated in f64."""
    y = ds.Y[rows].astype(np.float64)
    if ds.clip_outliers:
        y = np.clip(y, ds.min_vel, ds.max_vel)
    if ds.y_transform == "asinh":
        y = np.arcsinh(y / ds.y_scale)
    elif ds.y_transform == "signed_log":
        y = np.sign(y) * np.log1p(np.abs(y) / ds.y_scale)
    return 2 * (y - ds.trans_min) / (ds.trans_max - ds.trans_min) - 1.0


def _check_rows(ds, host, rows, x, y, m, what):
    """Device batch (x, y, m) == host items of ``rows``: mask exact, x within X_TOL, y within Y_TOL (asinh) or anchored in the
    host's own f32 error against the f64 formula (signed_log / none): e_dev <= 4 * e_host + 2^-23."""
    x, y, m = x.cpu(), y.cpu(), m.cpu()
    assert x.shape[0] == y.shape[0] == m.shape[0] == len(rows)
    hx, hy, hm = (torch.stack([host[r][k] for r in rows]) for k in range(3))
    assert torch.equal(m, hm), what
    torch.testing.assert_close(x, hx, **X_TOL, msg=lambda s: f"{what}: x: {s}")
    if ds.y_transform == "asinh":
        torch.testing.assert_close(y, hy, **Y_TOL, msg=lambda s: f"{what}: y: {s}")
        return None
    ref = _y64(ds, list(rows))
    e_host = float(np.abs(hy.numpy().astype(np.float64) - ref).max())
    e_dev = float(np.abs(y.numpy().astype(np.float64) - ref).max())
    print(f"[device_loader] {what}: max |y - f64|: host f32 {e_host:.3e}, device {e_dev:.3e} (bound 4 x host + 2^-23 = {4 * e_host + 2.0 ** -23:.3e})")
    assert e_dev <= 4 * e_host + 2.0 ** -23, (what, e_dev, e_host)
    return e_host, e_dev


def _index_vectors(n):
    return {"identity": None, "reversed": list(range(n - 1, -1, -1)), "repeats": [n - 1, 0, 0, n - 1, 1 % n, 0, n - 1],
            "single": [n // 2]}


# ---------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("case", CASES)
def test_kernel_matches_the_host_dataset_and_gather_is_bit_invariant(made, case, transform, clip):
    ds, host, xa, ya = made(case, transform, clip)
    n = len(ds)
    base = None
    for name, rows in _index_vectors(n).items():
        idx = None if rows is None else torch.tensor(rows, dtype=torch.int64, device=DEV)
        rows = list(range(n)) if rows is None else rows
        x, y, m = E._gather_transform(ds, xa, ya, idx, len(rows))
        _check_rows(ds, host, rows, x, y, m, f"{case} {transform} clip={clip} idx={name}")
        if base is None:
            base = (x, y, m)
            continue
        # a row produced through any index vector is bit-identical to the same row produced with idx = NULL
        for got, want in zip((x, y, m), base):
            assert torch.equal(got, want[idx]), (case, transform, clip, name)


def test_golden_fixture_matches_the_reference_items(made):
    g = load_golden("dataset")
    ds, host, xa, ya = made("golden", "asinh", True)
    x, y, m = E._gather_transform(ds, xa, ya, torch.tensor([1], dtype=torch.int64, device=DEV), 1)
    torch.testing.assert_close(x[0].cpu(), g["x1"], **X_TOL)              # the reference's own NPZSequenceDataset.__getitem__(1)
    torch.testing.assert_close(y[0].cpu(), g["y1"], **Y_TOL)
    assert torch.equal(m[0].cpu(), g["mask1"])


def test_a_bad_index_is_clamped_not_read(made):
    ds, host, xa, ya = made("5x7", "asinh", True)
    idx = torch.tensor([-3, len(ds) + 7, 2 ** 40], dtype=torch.int64, device=DEV)
    x, y, m = E._gather_transform(ds, xa, ya, idx, 3)
    _check_rows(ds, host, [0, len(ds) - 1, len(ds) - 1], x, y, m, "clamped")


@pytest.mark.parametrize("transform", ["signed_log", None, "none", "asinh"])
def test_device_transform_takes_every_transform(made, transform):
    for case in ("golden+edges", "5x7"):
        ds, host, xa, ya = made(case, transform, True)
        x, y, m = U.device_transform(ds, xa, ya)
        _check_rows(ds, host, list(range(len(ds))), x, y, m, f"device_transform {case} {transform}")


# ---------------------------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------------------------
N, B = 10, 4


@pytest.fixture(scope="module")
def ds10(tmp_path_factory):
    rng = np.random.default_rng(5)
    X = (rng.random((N, 2, 2, 4, 4)) * 30).astype(np.float32)
    X[:, 0, 0, 0, 0] = np.arange(N)                    # the row's own number, readable from a batch
    Y = rng.normal(0, 3, (N, 2, 1, 4, 4)).astype(np.float32)
    path = tmp_path_factory.mktemp("loader10") / "ds.npz"
    np.savez(path, X=X, Y=Y)
    return U.NPZSequenceDataset(str(path))


def _G(seed):
    return torch.Generator().manual_seed(seed)


def _rows_of(x, ds):
    return [int(round(float(v) * ds.norm_const)) for v in x[:, 0, 0, 0, 0].cpu()]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("which", ["dataset", "split0", "split1"])
def test_loader_equals_dataloader_over_the_same_sampler(ds10, which, drop_last):
    a, b = random_split(ds10, [7, 3], generator=_G(3))
    data = {"dataset": ds10, "split0": a, "split1": b}[which]
    host = DataLoader(data, batch_size=B, sampler=RandomSampler(data, generator=_G(7)), drop_last=drop_last)
    mine = U.DeviceSequenceLoader(data, B, sampler=RandomSampler(data, generator=_G(7)), drop_last=drop_last)
    assert len(mine) == len(host) and mine.dataset is data and mine.batch_size == B
    for epoch in range(3):
        want, got = list(host), list(mine)
        assert len(got) == len(want) == len(host)
        for (hx, hy, hm), (x, y, m) in zip(want, got):
            assert x.is_cuda and x.dtype == y.dtype == m.dtype == torch.float32 and x.is_contiguous()
            assert tuple(x.shape) == tuple(hx.shape) and tuple(y.shape) == tuple(hy.shape) == tuple(m.shape)
            assert _rows_of(x, ds10) == _rows_of(hx, ds10), (which, epoch)
            torch.testing.assert_close(x.cpu(), hx, **X_TOL)
            torch.testing.assert_close(y.cpu(), hy, **Y_TOL)
            assert torch.equal(m.cpu(), hm)
    # shuffle=True is RandomSampler(dataset, generator=generator)
    sh = U.DeviceSequenceLoader(data, B, shuffle=True, generator=_G(11), drop_last=drop_last)
    want = DataLoader(data, batch_size=B, sampler=RandomSampler(data, generator=_G(11)), drop_last=drop_last)
    assert [_rows_of(x, ds10) for x, _, _ in sh] == [_rows_of(x, ds10) for x, _, _ in want]


def test_one_resident_copy_for_all_loaders_of_a_dataset(ds10):
    a, b = random_split(ds10, [7, 3], generator=_G(3))
    la, lb, lw = U.DeviceSequenceLoader(a, B), U.DeviceSequenceLoader(b, B), U.DeviceSequenceLoader(ds10, B, shuffle=True)
    assert la.x_all.data_ptr() == lb.x_all.data_ptr() == lw.x_all.data_ptr()
    assert la.y_all.data_ptr() == lb.y_all.data_ptr() == lw.y_all.data_ptr()
    assert tuple(la.x_all.shape) == ds10.X.shape and torch.equal(la.x_all.cpu(), torch.from_numpy(ds10.X))
    assert torch.equal(la.y_all.cpu(), torch.from_numpy(ds10.Y))


def test_batches_write_into_static_buffers(ds10):
    T, C, H, W = ds10.X.shape[1:]
    out = (torch.empty(B, T, C, H, W, device=DEV), torch.empty(B, T, 1, H, W, device=DEV), torch.empty(B, T, 1, H, W, device=DEV))
    loader = U.DeviceSequenceLoader(ds10, B, drop_last=True)
    plain = [tuple(t.clone() for t in batch) for batch in loader]
    n = 0
    for k, (x, y, m) in enumerate(loader.batches(out=out)):
        assert x is out[0] and y is out[1] and m is out[2]
        for got, want in zip(out, plain[k]):
            assert torch.equal(got, want)
        n += 1
    assert n == len(plain) == N // B
    # a short last batch cannot go into the buffers; wrong shapes / CPU buffers are refused
    with pytest.raises(ValueError):
        U.DeviceSequenceLoader(ds10, B, drop_last=False).batches(out=out)
    with pytest.raises(ValueError):
        loader.batches(out=(out[0], out[1], torch.empty(B, T, 1, H, W + 1, device=DEV)))
    with pytest.raises(U.UclstmError):
        loader.batches(out=(out[0].cpu(), out[1], out[2]))
    # ... but drop_last=False is fine when the batches divide the epoch
    even = U.DeviceSequenceLoader(ds10, 5, drop_last=False)
    buf = tuple(torch.empty((5,) + tuple(t.shape[1:]), device=DEV) for t in out)
    assert sum(1 for _ in even.batches(out=buf)) == 2


def test_errors(ds10, tmp_path):
    path = tmp_path / "fresh.npz"
    np.savez(path, X=ds10.X, Y=ds10.Y)
    fresh = U.NPZSequenceDataset(str(path))                                 # nothing resident yet
    with pytest.raises(U.UclstmError) as e:
        U.DeviceSequenceLoader(fresh, B, max_resident_bytes=1)
    assert str(fresh.X.nbytes + fresh.Y.nbytes) in str(e.value) and " 1 bytes" in str(e.value)
    with pytest.raises(U.UclstmError):
        U.DeviceSequenceLoader(fresh, B, device="cpu")
    with pytest.raises(TypeError):
        U.DeviceSequenceLoader([1, 2, 3], B)
    with pytest.raises(IndexError):
        list(U.DeviceSequenceLoader(fresh, B, sampler=[0, N]))


def test_epoch_loops_take_the_device_loader(tmp_path):
    """The tiny set of test_gpu_data.py::test_train_one_epoch_and_evaluate_loops, fed from the device."""
    rng = np.random.default_rng(0)
    n, T, H, W = 8, 3, 32, 32
    X = (rng.random((n, T, 2, H, W)) * 30).astype(np.float32)
    X[X < 6] = 0.0
    Yv = np.tanh(X[:, :, :1] / 15.0 - 1.0).astype(np.float32) * 4.0
    path = tmp_path / "train.npz"
    np.savez(path, X=X, Y=Yv)
    ds = U.NPZSequenceDataset(str(path))
    loader = U.DeviceSequenceLoader(ds, 4)
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV)
    opt = U.FusedAdamW(model.parameters(), lr=2e-3, weight_decay=1e-4, max_grad_norm=1.0)
    hist = [U.train_one_epoch(model, loader, opt, torch.device(DEV), ds, use_mask=True) for _ in range(6)]
    for out in hist:
        assert len(out) == 4 and all(math.isfinite(v) for v in out)
    assert hist[-1][0] < hist[0][0], [h[0] for h in hist]
    ev = U.evaluate(model, loader, torch.device(DEV), ds, use_mask=True)
    ev_host = U.evaluate(model, DataLoader(ds, batch_size=4, shuffle=False), torch.device(DEV), ds, use_mask=True)
    assert len(ev) == 4 and all(math.isfinite(v) for v in ev)
    assert abs(ev[0] - ev_host[0]) <= 2e-2 * abs(ev_host[0]), (ev, ev_host)
    rep = U.evaluate_report(model, loader, torch.device(DEV), ds, use_mask=True)
    assert len(rep) == 5 and abs(rep[0] - ev[0]) <= 1e-4 * abs(ev[0])          # the same batches, the same weights
