"""GPU tests of DeviceNPZDataset: its constants against NPZSequenceDataset on the same file with ``==``, on every branch of the
host constructor; how many passes it launches; the shared resident copy; streaming a dataset that does not fit."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

DEV = "cuda"
CONSTANTS = ("x_max", "norm_const", "y_scale", "min_vel", "max_vel", "trans_min", "trans_max")
PCT = dict(min_y=None, max_y=None)                                      # the percentile branch, as the reference's main.py builds it


def _edges(X, Y):
    """The edge values tests/test_gpu_device_loader.py plants: targets outside the default [min_y, max_y], exact zeros of both
    signs, raw channel-0 values at float32(1.1) and its two neighbours."""
    t = np.float32(1.1)
    first, last, y = X[0, 0, 0].reshape(-1), X[-1, -1, 0].reshape(-1), Y.reshape(-1)
    first[:3] = [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(2))]
    last[-3:] = first[:3]
    y[:6] = [-20.0, 15.0, 0.0, -0.0, -7.6, 8.79]
    y[-4:] = [0.0, 40.0, -30.0, 1e-30]
    return X, Y


def _raw(case):
    if case == "golden":                                                # N = 3, T = 4, C = 2, 8 x 8
        g = load_golden("dataset")
        return _edges(g["X"].numpy().copy(), g["Y"].numpy().copy())
    rng = np.random.default_rng(len(case))
    N, T, C, H, W = {"5x7": (5, 1, 2, 5, 7), "c4": (4, 3, 4, 4, 8)}[case]
    X = (rng.random((N, T, C, H, W)) * 40).astype(np.float32)
    X[X < 8] = 0.0
    Y = (rng.standard_normal((N, T, 1, H, W)) * 3).astype(np.float32)
    if case == "c4":
        Y[rng.random(Y.shape) < 0.6] = 0.0                              # zero-heavy targets
    return _edges(X, Y)


CASES = ["golden", "5x7", "c4"]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    root = tmp_path_factory.mktemp("dataset_stats")
    out = {}
    for case in CASES:
        X, Y = _raw(case)
        out[case] = str(root / f"{case}.npz")
        np.savez(out[case], X=X, Y=Y)
    X, Y = _raw("5x7")
    Y[...] = np.float32(2.5)
    out["constant"] = str(root / "constant.npz")
    np.savez(out["constant"], X=X, Y=Y)
    X, Y = _raw("c4")
    Y.reshape(-1)[77] = np.nan
    out["nan"] = str(root / "nan.npz")
    np.savez(out["nan"], X=X, Y=Y)
    X, Y = _raw("c4")
    Y[...] = 0.0
    Y.reshape(-1)[[5, 200]] = [3.0, -2.0]                               # more than 99 % zeros: the percentile of |Y| is 0
    out["sparse"] = str(root / "sparse.npz")
    np.savez(out["sparse"], X=X, Y=Y)
    return out


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _agree(path, what, **kw):
    host, dev = U.NPZSequenceDataset(path, **kw), U.DeviceNPZDataset(path, **kw)
    for name in CONSTANTS:
        h, d = getattr(host, name), getattr(dev, name)
        assert type(d) is float and _same(h, d), (what, kw, name, h, d)
    assert (dev.N, dev.T, dev.H, dev.W, dev.y_transform, dev.clip_outliers) == (host.N, host.T, host.H, host.W, host.y_transform, host.clip_outliers)
    return host, dev


BRANCHES = {
    "percentiles": dict(PCT),
    "percentiles_25_75": dict(PCT, lower_percentile=25, upper_percentile=75),
    "explicit_min_max": dict(),                                         # the defaults: min_y / max_y given, y_scale from |Y|
    "explicit_scale": dict(PCT, y_transform_scale=2.5),
    "no_scale_percentile": dict(PCT, y_transform_percentile=None),
    "all_explicit": dict(y_transform_scale=1.75),
}


@pytest.mark.parametrize("branch", list(BRANCHES))
@pytest.mark.parametrize("case", CASES)
def test_constants_equal_the_host_constructor(paths, case, branch):
    for transform in ("asinh", "signed_log", None):
        host, dev = _agree(paths[case], (case, branch), y_transform=transform, **BRANCHES[branch])
        assert not any(math.isnan(getattr(host, n)) for n in CONSTANTS)
    for i in (0, len(dev) - 1):                                         # __getitem__ and denormalize are the parent's
        for a, b in zip(host[i], dev[i]):
            assert torch.equal(a, b)
    y = torch.linspace(-1, 1, 7)
    assert torch.equal(host.denormalize(y), dev.denormalize(y))


def test_a_constant_target_takes_the_plus_one_rule(paths):
    for transform in ("asinh", "signed_log", None):
        host, dev = _agree(paths["constant"], "constant", y_transform=transform, **PCT)
        assert dev.trans_max == dev.trans_min + 1.0 and dev.min_vel == dev.max_vel == 2.5


def test_a_nan_gives_nan_where_numpy_gives_nan(paths):
    for kw in (dict(PCT), dict(), dict(PCT, y_transform_scale=2.0)):
        host, dev = _agree(paths["nan"], "nan", **kw)
    assert math.isnan(dev.min_vel) and math.isnan(dev.trans_max) and not math.isnan(dev.y_scale) and not math.isnan(dev.x_max)
    host, dev = _agree(paths["nan"], "nan", **PCT)
    assert math.isnan(dev.y_scale)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_a_zero_scale_gives_numpys_nan(paths):
    """y_scale = 0 makes the transformed ARRAY 0 / 0 = NaN at every zero target, which its two order statistics do not show."""
    for transform in ("asinh", "signed_log", None):
        host, dev = _agree(paths["sparse"], "sparse", y_transform=transform, **PCT)
        assert dev.y_scale == 0.0 and -2.0 < dev.min_vel < 0.0 and math.isnan(dev.trans_min) == (transform is not None)


def test_launch_counts(paths):
    n_y = int(np.load(paths["c4"])["Y"].size)

    def passes(**kw):
        log = ops.LAUNCH_LOG = []
        try:
            U.DeviceNPZDataset(paths["c4"], **kw)
        finally:
            ops.LAUNCH_LOG = None
        return [e[2:] for e in log if e[:2] == ("select", "accumulate")], [e for e in log if e[0] == "extremes"]
    sel, ext = passes(**PCT)                                            # 6 order statistics, ONE select: three passes over Y
    assert sel == [(0, n_y), (1, n_y), (2, n_y)] and len(ext) == 1
    sel, ext = passes()
    assert sel == [(0, n_y), (1, n_y), (2, n_y)]
    sel, ext = passes(y_transform_scale=1.75)                           # nothing to select
    assert sel == [] and len(ext) == 1


def test_a_loader_reuses_the_resident_copy_and_yields_the_same_batches(paths):
    host, dev = _agree(paths["c4"], "c4", **PCT)
    (key, (x_dev, y_dev)), = dev._device_resident.items()
    loader = U.DeviceSequenceLoader(dev, 3)
    assert loader.x_all.data_ptr() == x_dev.data_ptr() and loader.y_all.data_ptr() == y_dev.data_ptr()
    assert list(dev._device_resident) == [key]
    ref = U.DeviceSequenceLoader(host, 3)
    assert ref.x_all.data_ptr() != x_dev.data_ptr()
    batches = list(zip(loader, ref))
    assert len(batches) == 2
    for got, want in batches:
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_a_dataset_that_does_not_fit_is_streamed(paths):
    for case in ("c4", "golden"):
        for kw in (dict(PCT), dict(PCT, y_transform="signed_log", lower_percentile=25, upper_percentile=75)):
            full = U.DeviceNPZDataset(paths[case], **kw)
            log = ops.LAUNCH_LOG = []
            try:
                ds = U.DeviceNPZDataset(paths[case], max_resident_bytes=1000, chunk_bytes=4 * 37 + 2, **kw)      # 37 elements: divides neither
            finally:
                ops.LAUNCH_LOG = None
            assert ds.Y.size % 37 and ds.X.size % 37
            for name in CONSTANTS:
                assert getattr(ds, name) == getattr(full, name), (case, name)
            assert not ds.__dict__.get("_device_resident")
            per_pass = -(-ds.Y.size // 37)
            assert [e[2] for e in log if e[:2] == ("select", "accumulate")] == [0] * per_pass + [1] * per_pass + [2] * per_pass
            with pytest.raises(U.UclstmError, match="does not fit"):
                U.DeviceSequenceLoader(ds, 2, max_resident_bytes=1000)
            assert not ds.__dict__.get("_device_resident")


def test_exact_percentile_is_the_f64_rank(paths):
    rng = np.random.default_rng(11)
    v = (rng.standard_normal(1001) * 3).astype(np.float32)
    t = torch.from_numpy(v).to(DEV)
    s = np.sort(v).astype(np.float64)
    for absolute in (False, True):
        s = np.sort(np.abs(v) if absolute else v).astype(np.float64)
        for q in (0.0, 37.3, 50.0, 99.99999, 100.0):
            vi = (v.size - 1) * (q / 100.0)
            lo = min(int(math.floor(vi)), v.size - 1)
            hi, g = min(lo + 1, v.size - 1), vi - lo
            want = s[lo] + (s[hi] - s[lo]) * g if g < 0.5 else s[hi] - (s[hi] - s[lo]) * (1 - g)
            assert U.device_percentile(t, q, absolute=absolute, exact=True) == want, (q, absolute)
            assert U.device_percentile(t, q, absolute=absolute) == float(np.percentile(np.abs(v) if absolute else v, q)), (q, absolute)
    assert U.device_percentile(t, [12.5, 99.0]) == [float(np.percentile(v, 12.5)), float(np.percentile(v, 99.0))]
