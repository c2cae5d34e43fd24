"""GPU tests of the device-side evaluation report (uclstm_eval_stats / EvalReport / evaluate_report / tools/eval_report.py)
against the numpy formulas of train/get_metrics.py and test.py, restated here on seeded inputs.

Bounds.  Sums: 1e-5 relative, the tolerance of test_gpu_data.py::test_metric_sums_match_main_py_formulas (a signed sum is
compared relative to the sum of the magnitudes it adds: that is what its rounding scales with).  Values (min / max, bin
membership): DELTA = 1e-4 m/s absolute, 20 x the f32-vs-f64 de-normalisation difference at |v| <= 8.8 (5.3e-6); a count may
differ from numpy's on f64 values by at most the number of f64 values within DELTA of one of the bin's edges."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L

DEV = "cuda"
DELTA = 1e-4


class _DS:
    """The attributes of NPZSequenceDataset that de-normalisation reads, with its denormalize() for numpy input."""

    def __init__(self, y_transform, y_scale, trans_min, trans_max):
        self.y_transform, self.y_scale, self.trans_min, self.trans_max = y_transform, float(y_scale), float(trans_min), float(trans_max)

    def denormalize(self, y_norm):
        return U.NPZSequenceDataset.denormalize(self, y_norm)


def _dataset(y_transform="asinh", y_scale=2.0, min_y=-7.5987958908081055, max_y=8.784920692443848):
    """trans_min / trans_max as NPZSequenceDataset.__init__ derives them from explicit min_y / max_y (the defaults)."""
    fwd = {"asinh": lambda v: np.arcsinh(v / y_scale), "signed_log": lambda v: np.sign(v) * np.log1p(np.abs(v) / y_scale),
           None: lambda v: v}[y_transform]
    return _DS(y_transform, y_scale, float(fwd(np.float64(min_y))), float(fwd(np.float64(max_y))))


def _denorm64(ds, v):
    return ds.denormalize(np.asarray(v, dtype=np.float64))


def _as_model_output(t):
    """[B,T,...] values laid out as the model returns them: a transposed view of a [T,B,...] buffer."""
    buf = t.transpose(0, 1).contiguous().to(DEV)
    view = buf.transpose(0, 1)
    assert not view.is_contiguous() or t.shape[0] == 1 or t.shape[1] == 1
    return view


def _rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.abs(b) if scale is None else np.asarray(scale, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(s, 1e-300))) if a.size else 0.0


def _inputs(shape, seed, bias=0.02):
    rng = np.random.default_rng(seed)
    y = rng.uniform(-1, 1, shape).astype(np.float32)
    yp = (y + 0.1 * rng.standard_normal(shape) + bias).astype(np.float32)
    mask = (rng.random(shape) > 0.4).astype(np.float32)
    return y, yp, mask


# ---------------------------------------------------------------------------------------------
# 1. sums
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 1, 64, 64), (2, 3, 2, 40, 40), (2, 5, 1, 7, 9), (2, 3, 1, 47, 47), (2, 2, 1, 256, 256)],
                         ids=["64x64", "C2_40x40", "odd_7x9", "odd_47x47_two_chunks", "256x256"])
@pytest.mark.parametrize("y_transform", ["asinh", "signed_log", None])
@pytest.mark.parametrize("use_mask", [True, False])
def test_sums_global_per_timestep_per_sequence(shape, y_transform, use_mask):
    ds = _dataset(y_transform)
    rep = U.EvalReport(ds, device=DEV)
    parts = [_inputs(shape, 3), _inputs(shape, 4)]
    for y, yp, mask in parts:
        view = _as_model_output(torch.from_numpy(yp))
        rep.add(torch.from_numpy(y).to(DEV), view, torch.from_numpy(mask).to(DEV), use_mask)
        assert rep.last_pointers[0] == view.data_ptr() and not view.is_contiguous() and rep.last_copies == 0       # read in place, no copy
    r = rep.result()
    y, yp, mask = (np.concatenate(a, axis=0) for a in zip(*parts))
    gt, pr = ds.denormalize(y).astype(np.float64), ds.denormalize(yp).astype(np.float64)   # the dataset's own f32 denormalize
    assert ds.denormalize(y).dtype == np.float32
    valid = mask != 0 if use_mask else np.ones(y.shape, dtype=bool)
    d = pr - gt
    D = d[valid]
    N, T = y.shape[:2]
    P = int(np.prod(shape[2:]))
    if P % 4:
        assert shape[3] * shape[4] % 4 != 0
    fig = {"n": (r["n"], D.size), "mae": (r["mae"], np.abs(D).mean()), "rmse": (r["rmse"], math.sqrt((D ** 2).mean())),
           "mean_err": (r["mean_err"], D.mean()), "std_err": (r["std_err"], D.std()),
           "gt_mean": (r["gt_mean"], gt[valid].mean()), "gt_std": (r["gt_std"], gt[valid].std()),
           "pred_mean": (r["pred_mean"], pr[valid].mean()), "pred_std": (r["pred_std"], pr[valid].std())}
    for k, (got, want) in fig.items():
        print(f"[eval_report sums] {k}: device {got!r} host {float(want)!r} rel {_rel(got, want):.2e}")
    assert r["n"] == D.size
    for k in ("mae", "rmse", "std_err", "gt_std", "pred_std"):
        assert _rel(*fig[k]) <= 1e-5, (k, fig[k])
    for k, mag in (("mean_err", np.abs(D).mean()), ("gt_mean", np.abs(gt[valid]).mean()), ("pred_mean", np.abs(pr[valid]).mean())):
        assert _rel(*fig[k], scale=mag) <= 1e-5, (k, fig[k])
    # per time step (get_metrics.py:281-297: time index = axis 1) and per frame (test.py:333-351)
    w = valid.astype(np.float64)
    axes_t, axes_f = (0, 2, 3, 4), (2, 3, 4)
    for name, axes, got in (("per_timestep", axes_t, None), ("per_sequence", axes_f, r["per_sequence"])):
        n_ = w.sum(axis=axes)
        sa, sq, sd = (np.abs(d) * w).sum(axis=axes), (d * d * w).sum(axis=axes), (d * w).sum(axis=axes)
        if got is None:
            pt = r["per_timestep"]
            assert np.array_equal(pt["n"], n_)
            e = (_rel(pt["mae"], sa / n_), _rel(pt["rmse"], np.sqrt(sq / n_)), _rel(pt["mean_err"], sd / n_, scale=sa / n_))
        else:
            assert got.shape == (N, T, 4) and np.array_equal(got[..., 0], n_)
            e = (_rel(got[..., 1], sa), _rel(got[..., 2], sq), _rel(got[..., 3], sd, scale=sa))
        print(f"[eval_report sums] {name}: worst relative difference of (|d|, d^2, d) sums {e}")
        assert max(e) <= 1e-5, (name, e)


# ---------------------------------------------------------------------------------------------
# 2. + 3. min / max, histograms, digitize counts on the issue's inputs
# ---------------------------------------------------------------------------------------------
def _issue_inputs():
    rng = np.random.default_rng(5)
    shape = (4, 6, 1, 64, 64)
    y = rng.uniform(-1, 1, shape).astype(np.float32)
    yp = np.clip(y + 0.15 * rng.standard_normal(shape), -1.2, 1.2).astype(np.float32)
    return y, yp


def _near_edges(x, edges):
    """near[e]: number of values within DELTA of edge e."""
    srt = np.sort(x)
    return np.searchsorted(srt, edges + DELTA, side="right") - np.searchsorted(srt, edges - DELTA, side="left")


def _check_hist(name, got, x, bins, rng_):
    want, edges = np.histogram(x, bins, rng_)
    ne = _near_edges(x, edges)
    near = ne[:-1] + ne[1:]
    diff = np.abs(got.astype(np.int64) - want)
    share = ne.sum() / x.size
    outside = float(np.mean((x < rng_[0]) | (x > rng_[1])))
    print(f"[eval_report hist] {name}: bins that differ {int((diff > 0).sum())}, largest difference {int(diff.max())}, "
          f"values within DELTA of an edge {100 * share:.3f} %, outside the range {100 * outside:.2f} %")
    assert share <= 0.01, (name, share)                             # the condition under which the bound says something
    assert 0.03 <= outside <= 0.10, (name, outside)                 # the drop rule is exercised
    assert np.all(diff <= near), (name, np.nonzero(diff > near)[0], diff[diff > near], near[diff > near])
    assert abs(int(got.sum()) - int(want.sum())) <= ne[0] + ne[-1], (name, int(got.sum()), int(want.sum()))


def _check_digitize(name, got, x, edges):
    want = np.bincount(np.digitize(x, edges), minlength=len(edges) + 1)
    ne = _near_edges(x, edges)
    near = np.concatenate(([ne[0]], ne[:-1] + ne[1:], [ne[-1]]))
    diff = np.abs(got.astype(np.int64) - want)
    share = ne.sum() / x.size
    print(f"[eval_report hist] {name}: bins that differ {int((diff > 0).sum())}, largest difference {int(diff.max())}, "
          f"values within DELTA of an edge {100 * share:.3f} %")
    assert share <= 0.01, (name, share)
    assert got.sum() == x.size and len(got) == len(edges) + 1
    assert np.all(diff <= near), (name, np.nonzero(diff > near)[0])


def test_min_max_histograms_and_digitize_counts():
    ds = _dataset("asinh", y_scale=2.0)
    y, yp = _issue_inputs()
    rep = U.EvalReport(ds, device=DEV)
    rep.add(torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)))
    r = rep.result()
    gt, pr = _denorm64(ds, y).ravel(), _denorm64(ds, yp).ravel()     # host f64
    d = pr - gt
    worst = 0.0
    for k, want in (("gt_min", gt.min()), ("gt_max", gt.max()), ("pred_min", pr.min()), ("pred_max", pr.max()),
                    ("err_min", d.min()), ("err_max", d.max())):
        worst = max(worst, abs(r[k] - want))
        print(f"[eval_report minmax] {k}: device {r[k]!r} host f64 {float(want)!r} difference {r[k] - want:+.3e}")
    print(f"[eval_report minmax] largest device-minus-host difference {worst:.3e} (DELTA {DELTA})")
    assert worst <= DELTA
    _check_hist("gt", r["hist_gt"], gt, 100, (-7.5, 7.5))
    _check_hist("pred", r["hist_pred"], pr, 100, (-7.5, 7.5))
    _check_hist("err", r["hist_err"], d, 100, (-3.0, 3.0))
    _check_digitize("digitize", r["gt_bin_count"], gt, r["scatter_edges"])
    assert np.array_equal(r["hist_edges"], np.histogram(gt, 100, (-7.5, 7.5))[1])


# ---------------------------------------------------------------------------------------------
# 4. skew
# ---------------------------------------------------------------------------------------------
def _skewed(shape, seed, share=0.85, value=-0.4137):
    rng = np.random.default_rng(seed)
    y = rng.uniform(-1, 1, shape).astype(np.float32)
    y[rng.random(shape) < share] = value                            # background pixels share one target value
    yp = np.clip(y + 0.05 * rng.standard_normal(shape), -1.2, 1.2).astype(np.float32)
    return y, yp


@pytest.mark.parametrize("share", [0.85, 1.0])
def test_skewed_targets_give_numpy_counts(share):
    ds = _dataset("asinh", y_scale=2.0)
    y, yp = _skewed((2, 3, 1, 64, 64), 8, share)
    mask = (np.random.default_rng(9).random(y.shape) > 0.2).astype(np.float32)
    rep = U.EvalReport(ds, device=DEV)
    rep.add(torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)), torch.from_numpy(mask).to(DEV), True)
    r = rep.result()
    v = mask != 0
    gt, pr = _denorm64(ds, y)[v], _denorm64(ds, yp)[v]
    edges = r["scatter_edges"]
    top = np.bincount(np.digitize(gt, edges)).max() / gt.size
    assert top >= share - 0.01
    for name, got, x, rng_ in (("gt", r["hist_gt"], gt, (-7.5, 7.5)), ("pred", r["hist_pred"], pr, (-7.5, 7.5)),
                               ("err", r["hist_err"], pr - gt, (-3.0, 3.0))):
        want, e = np.histogram(x, 100, rng_)
        ne = _near_edges(x, e)
        assert np.all(np.abs(got - want) <= ne[:-1] + ne[1:]), name
    want = np.bincount(np.digitize(gt, edges), minlength=len(edges) + 1)
    ne = _near_edges(gt, edges)
    near = np.concatenate(([ne[0]], ne[:-1] + ne[1:], [ne[-1]]))
    assert np.all(np.abs(r["gt_bin_count"] - want) <= near)
    b = int(np.argmax(want))                                        # the background value sits well inside its bin: exact
    assert near[b] < want[b] * 1e-3 + 50 and abs(int(r["gt_bin_count"][b]) - int(want[b])) <= near[b]
    assert r["gt_bin_count"].sum() == gt.size == r["n"]


def test_counters_that_just_fit_the_lds_budget_give_numpy_counts():
    """4096 bins and 1022 edges: 3 * 4096 + 3 * 1023 = 15 357 of the 15 360 counters that 60 KiB hold, the largest configuration
    whose counters stay in LDS, all of it the one channel's region.  No transform and [-1, 1] -> [-1, 1], so the device's f32 values
    are numpy's bit for bit (_identity_dataset), and ranges whose edges are exact in binary (steps 2^-11, 2^-14 and 2^-9), so a
    value on an edge falls to the same side in both: the counts are np.histogram's and np.digitize's on the f64 of those f32
    values, compared with ==."""
    ds = _identity_dataset()
    shape = (2, 3, 1, 47, 47)
    y, yp = _skewed(shape, 8)                                        # 85 % of the targets share one value: count_in_lds's leader adds
    kw = dict(hist_bins=4096, hist_range=(-1.0, 1.0), err_range=(-0.125, 0.125), scatter_range=(-1.0, -1.0 + 1021 / 512),
              scatter_bin_width=1 / 512)
    rep = U.EvalReport(ds, points_per_bin=4, device=DEV, **kw)
    edges = rep.scatter_edges
    assert len(edges) == 1022 and 3 * 4096 + 3 * (len(edges) + 1) == 15357 <= 15 * 1024
    rep.add(torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)))
    r = rep.result()
    g32, p32 = ds.denormalize(y), ds.denormalize(yp)
    assert g32.dtype == np.float32 and p32.dtype == np.float32
    gt, pr, d = g32.astype(np.float64).ravel(), p32.astype(np.float64).ravel(), (p32 - g32).astype(np.float64).ravel()
    want = np.bincount(np.digitize(gt, edges), minlength=len(edges) + 1)
    assert want.max() >= 0.84 * gt.size
    for name, got, x, rng_ in (("gt", r["hist_gt"], gt, kw["hist_range"]), ("pred", r["hist_pred"], pr, kw["hist_range"]),
                               ("err", r["hist_err"], d, kw["err_range"])):
        ref = np.histogram(x, 4096, rng_)[0]
        print(f"[eval_report budget] {name}: bins that differ {int((got != ref).sum())}, counted {int(got.sum())} of {x.size}, "
              f"non-empty bins {int((ref > 0).sum())}")
        assert np.array_equal(got, ref), (name, np.nonzero(got != ref)[0])
    assert 0 < r["hist_pred"].sum() < pr.size and 0 < r["hist_err"].sum() < d.size                   # the drop rule is exercised
    print(f"[eval_report budget] digitize: bins that differ {int((r['gt_bin_count'] != want).sum())}, non-empty bins {int((want > 0).sum())}")
    assert np.array_equal(r["gt_bin_count"], want)
    assert np.array_equal(np.bincount(r["scatter_bin"], minlength=len(want)), np.minimum(want, 4))


def test_counters_beyond_the_lds_budget_use_the_global_path():
    """4096 bins and 20001 edges do not fit the per-block LDS counters: same figures through per-pixel integer atomics."""
    ds = _dataset("asinh", y_scale=2.0)
    y, yp, mask = _inputs((2, 2, 1, 32, 32), 21)
    kw = dict(hist_bins=4096, scatter_range=(-8.0, 8.0), scatter_bin_width=0.0008, points_per_bin=3)
    rep = U.EvalReport(ds, device=DEV, **kw)
    assert 3 * 4096 + 3 * (len(rep.scatter_edges) + 1) > 15 * 1024
    rep.add(torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)), torch.from_numpy(mask).to(DEV), True)
    r = rep.result()
    v = mask != 0
    gt = _denorm64(ds, y)[v]
    want, e = np.histogram(gt, 4096, (-7.5, 7.5))
    ne = _near_edges(gt, e)
    assert np.all(np.abs(r["hist_gt"] - want) <= ne[:-1] + ne[1:])
    wd = np.bincount(np.digitize(gt, rep.scatter_edges), minlength=len(rep.scatter_edges) + 1)
    ne = _near_edges(gt, rep.scatter_edges)
    assert np.all(np.abs(r["gt_bin_count"] - wd) <= np.concatenate(([ne[0]], ne[:-1] + ne[1:], [ne[-1]])))
    assert r["n"] == gt.size and len(r["scatter_gt"]) == int(np.minimum(r["gt_bin_count"], 3).sum())
    d = (ds.denormalize(yp).astype(np.float64) - ds.denormalize(y).astype(np.float64))[v]
    assert _rel(r["mae"], np.abs(d).mean()) <= 1e-5


# ---------------------------------------------------------------------------------------------
# 5. scatter sample
# ---------------------------------------------------------------------------------------------
def _identity_dataset():
    """No transform and [-1, 1] -> [-1, 1]: de-normalisation is fl(fl(v + 1) - 1) on the device and in numpy alike, so a
    stored pair can be matched to its input pixel bit for bit."""
    return _DS(None, 1.0, -1.0, 1.0)


def _keys(gt, pr):
    return (np.ascontiguousarray(gt, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.ascontiguousarray(pr, dtype=np.float32).view(np.uint32).astype(np.uint64)


def test_scatter_sample_holds_input_pixels_and_fills_every_bin():
    ds = _identity_dataset()
    K = 200
    rng = np.random.default_rng(12)
    shape = (3, 4, 1, 48, 48)
    rep = U.EvalReport(ds, scatter_range=(-0.8, 0.8), scatter_bin_width=0.01, points_per_bin=K, seed=7, device=DEV)
    keys, gts = [], []
    for _ in range(2):
        y = rng.normal(0.0, 0.45, shape).astype(np.float32)          # dense bins in the middle, sparse ones outside, under/overflow
        yp = (y + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        mask = (rng.random(shape) > 0.3).astype(np.float32)
        rep.add(torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)), torch.from_numpy(mask).to(DEV), True)
        g, p = ds.denormalize(y), ds.denormalize(yp)
        assert g.dtype == np.float32
        keys.append(_keys(g[mask != 0], p[mask != 0]))
        gts.append(g[mask != 0])
    r = rep.result()
    raw = rep._scatter.cpu().numpy()
    edges, cnt = r["scatter_edges"], r["gt_bin_count"]
    gt_all = np.concatenate(gts).astype(np.float64)
    ne = _near_edges(gt_all, edges)
    near = np.concatenate(([ne[0]], ne[:-1] + ne[1:], [ne[-1]]))
    assert np.all(np.abs(cnt - np.bincount(np.digitize(gt_all, edges), minlength=len(edges) + 1)) <= near)
    assert cnt.sum() == gt_all.size and (cnt > K).sum() >= 20 and ((cnt > 0) & (cnt < K)).sum() >= 5
    # per bin: filled slots = min(count, K); nothing beyond them was written
    fill = np.minimum(cnt, K)
    assert np.array_equal(np.bincount(r["scatter_bin"], minlength=len(cnt)), fill)
    pool = np.unique(np.concatenate(keys))
    stored = _keys(r["scatter_gt"], r["scatter_pred"])
    assert np.all(np.isin(stored, pool)), "a stored pair is not the (gt, pred) of a valid input pixel"
    for b in range(len(cnt)):
        assert not raw[b, fill[b]:].any(), b
    # ... and every stored gt lies in its bin, up to DELTA
    lo = np.concatenate(([-np.inf], edges))[r["scatter_bin"]]
    hi = np.concatenate((edges, [np.inf]))[r["scatter_bin"]]
    g = r["scatter_gt"].astype(np.float64)
    assert np.all((g >= lo - DELTA) & (g < hi + DELTA))
    # a saturated bin holds K DIFFERENT pixels only if replacement works on whole pairs: no slot mixes two pixels (checked
    # above through the pool) and the sample is not K copies of one pixel
    b = int(np.argmax(cnt))
    assert len(np.unique(stored[r["scatter_bin"] == b])) > K // 2


def test_scatter_sample_is_uniform_over_add_calls():
    """K = 1000, four add() calls that each put >= 5000 pixels into ONE bin: reservoir sampling keeps ~25 % from each
    (binomial sigma 1.4 %); keeping the first K would give 100 / 0 / 0 / 0."""
    ds = _identity_dataset()
    K = 1000
    rng = np.random.default_rng(13)
    shape = (2, 3, 1, 32, 32)                                        # 6144 pixels per call
    rep = U.EvalReport(ds, points_per_bin=K, seed=3, device=DEV)
    for call in range(4):
        y = rng.uniform(0.51, 0.54, shape).astype(np.float32)        # one bin of width 0.05: [0.5, 0.55)
        yp = (0.1 * call + rng.uniform(0.0, 0.05, shape)).astype(np.float32)       # the prediction tells the call
        rep.add(torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)))
    r = rep.result()
    b = int(np.digitize(0.525, r["scatter_edges"]))
    assert r["gt_bin_count"][b] == 4 * 6144 and r["gt_bin_count"].sum() == 4 * 6144
    pred = r["scatter_pred"][r["scatter_bin"] == b]
    assert len(pred) == K
    share = [float(np.mean((pred >= 0.1 * c - 1e-3) & (pred < 0.1 * c + 0.05 + 1e-3))) for c in range(4)]
    print(f"[eval_report scatter] share of the bin's sample per add() call: {share}")
    assert abs(sum(share) - 1.0) < 1e-9
    assert all(0.10 <= s <= 0.40 for s in share), share


# ---------------------------------------------------------------------------------------------
# 6. reproducibility
# ---------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal_except_the_sample():
    ds = _dataset("asinh", y_scale=2.0)
    y, yp = _issue_inputs()
    mask = (np.random.default_rng(6).random(y.shape) > 0.3).astype(np.float32)
    runs = []
    for _ in range(2):
        rep = U.EvalReport(ds, device=DEV)
        for h in (slice(0, 2), slice(2, 4)):
            rep.add(torch.from_numpy(y[h]).to(DEV), _as_model_output(torch.from_numpy(yp[h])), torch.from_numpy(mask[h]).to(DEV), True)
        runs.append(rep.result())
    a, b = runs

    def same(u, v, key):
        if isinstance(u, dict):
            for k in u:
                same(u[k], v[k], f"{key}.{k}")
        elif isinstance(u, np.ndarray):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), key
        else:
            assert np.float64(u).tobytes() == np.float64(v).tobytes(), key

    assert set(a) == set(b)
    for k in a:
        if k not in ("scatter_gt", "scatter_pred"):
            same(a[k], b[k], k)
    assert len(a["scatter_gt"]) == len(b["scatter_gt"])


# ---------------------------------------------------------------------------------------------
# 7. evaluate_report, 8. the tool
# ---------------------------------------------------------------------------------------------
def _tiny_npz(path, N=8):
    rng = np.random.default_rng(0)
    T, H, W = 3, 32, 32
    X = (rng.random((N, T, 2, H, W)) * 30).astype(np.float32)
    X[X < 6] = 0.0
    Yv = np.tanh(X[:, :, :1] / 15.0 - 1.0).astype(np.float32) * 4.0
    np.savez(path, X=X, Y=Yv)


def test_evaluate_report_returns_what_evaluate_returns(tmp_path, monkeypatch):
    """evaluate_report's first four values are evaluate()'s computation: EXACTLY the loss accumulation and the `_Metrics` of
    evaluate() over the very launches of its own loop (the `_Metrics` instance it used is captured and asked again), and equal
    to a separate evaluate() pass up to what evaluate() can reproduce of itself.  evaluate() is not bitwise equal to itself
    from run to run: its loss and metric kernels combine <= 1024 block partials with f64 atomic adds in arrival order.  Each
    of those sums of B partials carries a relative rounding error <= B * 2^-53 (1.1e-13 at B = 1024) of the sum of
    magnitudes, so two passes differ by <= 1e-12 relative in mae / rmse (mean_err: of mae, the scale of what it adds); the
    loss is rounded to f32 per batch, where such a difference can flip at most the last bit: 2^-23 relative."""
    from unet_convlstm_amd import engine
    path = tmp_path / "train.npz"
    _tiny_npz(path)
    ds = U.NPZSequenceDataset(str(path))
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV)
    opt = U.FusedAdamW(model.parameters(), lr=2e-3, weight_decay=1e-4, max_grad_norm=1.0)
    U.train_one_epoch(model, loader, opt, torch.device(DEV), ds, use_mask=True)
    seen = []

    class Spy(engine._Metrics):
        def __init__(self, device):
            super().__init__(device)
            seen.append(self)

    for use_mask in (True, False):
        ev = U.evaluate(model, loader, torch.device(DEV), ds, use_mask=use_mask)
        del seen[:]
        with monkeypatch.context() as mp:
            mp.setattr(engine, "_Metrics", Spy)
            out = U.evaluate_report(model, loader, torch.device(DEV), ds, use_mask=use_mask)
        assert len(out) == 5 and len(seen) == 1
        # _Metrics.result() only reads the sums back (no reset, no accumulation), so asking the captured instance a second time
        # returns what evaluate_report got from it
        assert tuple(out[1:4]) == tuple(seen[0].result())              # the same launches: exact
        rep = out[4]
        print(f"[eval_report evaluate] use_mask={use_mask}: evaluate {ev}, evaluate_report {out[:4]}, "
              f"report {(rep['mae'], rep['rmse'], rep['mean_err'])}")
        assert abs(out[0] - ev[0]) <= 2.0 ** -23 * abs(ev[0]), (out[0], ev[0])
        assert _rel(out[1], ev[1]) <= 1e-12 and _rel(out[2], ev[2]) <= 1e-12 and _rel(out[3], ev[3], scale=ev[1]) <= 1e-12, (out[:4], ev)
        assert _rel(rep["mae"], ev[1]) <= 1e-5 and _rel(rep["rmse"], ev[2]) <= 1e-5 and _rel(rep["mean_err"], ev[3]) <= 1e-5
        assert rep["per_sequence"].shape == (8, 3, 4) and rep["n"] == rep["per_sequence"][..., 0].sum()


def test_tool_writes_the_report(tmp_path):
    npz, ckpt, out = tmp_path / "data.npz", tmp_path / "model.pt", tmp_path / "report.npz"
    _tiny_npz(npz, N=10)
    torch.manual_seed(1)
    model = U.TemporalUNetDualView(1, 1, base_ch=8, lstm_layers=1, use_skip_lstm=True, use_attention=False)
    torch.save({"config": {"type": "custom", "base_ch": 8, "use_skip_lstm": True, "use_attention": False},
                "model_state": model.state_dict()}, ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_report.py"), "--checkpoint", str(ckpt), "--npz", str(npz),
           "--batch", "2", "--use-mask", "--out", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for line in ("Global MAE:", "Global RMSE:", "Global Mean Error (Bias):", "Global Error Std:"):
        assert line in p.stdout, p.stdout
    # the same split and model here (get_metrics.py:97-106)
    ds = U.NPZSequenceDataset(str(npz), min_y=None, max_y=None)
    n_train = int(0.8 * len(ds))
    _, val = torch.utils.data.random_split(ds, [n_train, len(ds) - n_train], generator=torch.Generator().manual_seed(42))
    loader = torch.utils.data.DataLoader(val, batch_size=2, shuffle=False)
    want = U.evaluate(model.to(DEV), loader, torch.device(DEV), ds, use_mask=True)
    with np.load(out, allow_pickle=False) as z:
        got = {k: z[k] for k in z.files}
    assert _rel(got["mae"], want[1]) <= 1e-5 and _rel(got["rmse"], want[2]) <= 1e-5
    assert got["per_sequence"].shape == (len(val), 3, 4) and got["hist_gt"].shape == (100,) and got["gt_bin_count"].shape == (322,)
