"""GPU tests of the vector evaluation report (uclstm_eval_stats_vec / VectorEvalReport / evaluate_vector_report /
tools/eval_report.py --axes).

Per channel the yardstick is the scalar kernel itself: channel c's table rows, histogram counts and digitize counts are compared
with ``==`` against uclstm_eval_stats pointed at channel c in place, and every pair the scatter sample keeps must be one of the
pairs the scalar kernel produces for that channel and bin (the scalar report run with room for every pair).

Vector part, against f64 numpy on the dataset's own f32 denormalize.  Bounds: sums 1e-5 relative, the project's sum bound (a
signed sum relative to the sum of the magnitudes it adds); values (bin membership, epe of the constructed field) DELTA = 1e-4 m/s,
the constant of tests/test_gpu_eval_report.py; angles DTHETA = 0.01 degrees: two vectors whose components each carry at most the
5.3e-6 m/s de-normalisation difference quoted there turn, at speed >= 0.5 m/s, by <= 3e-5 rad = 1.7e-3 degrees, times 6.  A sum
of n angles may differ by n * DTHETA, a sum of n squared angles by n * 360 * DTHETA (|x^2 - y^2| = |x - y| |x + y|, |x + y| <= 360).

Measured on an MI355X (asinh, mask, [2,3,3,47,47]): see profiles/eval_report_vec.txt."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import vector_cases as VC
from vector_report_cases import vector_dataset, vector_quantities, sign

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U

DEV = "cuda"
DELTA = 1e-4
DTHETA = 0.01
MIN_SPEED = 0.5
TRANSFORMS = ["asinh", "signed_log", None]


class _One:
    """Channel c of a vector dataset as the scalar dataset EvalReport takes."""

    def __init__(self, ds, c):
        self.y_transform, self.y_scale, self.trans_min, self.trans_max = ds.y_transform, float(ds.y_scale[c]), float(ds.trans_min[c]), float(ds.trans_max[c])


def _as_model_output(t):
    """[B,T,...] values laid out as the model returns them: a transposed view of a [T,B,...] buffer."""
    return t.transpose(0, 1).contiguous().to(DEV).transpose(0, 1)


def _rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.abs(b) if scale is None else np.asarray(scale, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(s, 1e-300))) if a.size else 0.0


def _keys(gt, pr):
    return (np.ascontiguousarray(gt, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.ascontiguousarray(pr, dtype=np.float32).view(np.uint32).astype(np.uint64)


def _pairs(r):
    return set(zip(r["scatter_bin"].tolist(), _keys(r["scatter_gt"], r["scatter_pred"]).tolist()))


def _bits(t):
    return t.contiguous().cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed):
    rng = np.random.default_rng(seed)
    B, T, Cy, H, W = shape
    y = rng.uniform(-1, 1, shape).astype(np.float32)
    yp = (y + 0.1 * rng.standard_normal(shape) + 0.02).astype(np.float32)
    mask = (rng.random((B, T, 1, H, W)) > 0.4).astype(np.float32)
    return y, yp, mask


def _scalar_in_place(ds, c, y_d, view, m_d, use_mask, K, **kw):
    """uclstm_eval_stats on channel c of the very tensors the vector kernel read: base + c * HW, the same strides, the one-channel mask."""
    rep = U.EvalReport(_One(ds, c), points_per_bin=K, device=DEV, **kw)
    rep.add(y_d[:, :, c:c + 1], view[:, :, c:c + 1], m_d, use_mask)
    HW = y_d.shape[3] * y_d.shape[4]
    assert rep.last_copies == 0 and rep.last_pointers[:2] == (view.data_ptr() + 4 * c * HW, y_d.data_ptr() + 4 * c * HW)
    return rep


def _check_channels_equal_the_scalar_kernel(ds, rep, r, y_d, view, m_d, use_mask, K, pool=True, **kw):
    table, hist, dig = rep._tables[0][0], rep._hist, rep._dig
    for c in range(ds.Cy):
        cnt = r["channels"][c]["gt_bin_count"]
        ref = _scalar_in_place(ds, c, y_d, view, m_d, use_mask, max(int(cnt.max()), 1) if pool else K, **kw)
        assert _bits(table[:, c]) == _bits(ref._tables[0][0]), f"channel {c}: table rows"
        assert torch.equal(hist[c], ref._hist) and torch.equal(dig[c], ref._dig), f"channel {c}: counts"
        ch = r["channels"][c]
        assert np.array_equal(np.bincount(ch["scatter_bin"], minlength=len(cnt)), np.minimum(cnt, K)), f"channel {c}: scatter fill"
        raw = rep._scatter[c].cpu().numpy()
        fill = np.minimum(cnt, K)
        assert not any(raw[b, fill[b]:].any() for b in np.nonzero(fill < K)[0]), f"channel {c}: a slot beyond the fill count was written"
        if pool:
            rr = ref.result()
            assert len(rr["scatter_gt"]) == int(cnt.sum())             # the scalar report kept every pair of every bin
            assert _pairs(ch) <= _pairs(rr), f"channel {c}: a kept pair is not a (gt, pred) pair of that channel and bin"


# ---------------------------------------------------------------------------------------------
# 1. bit for bit per channel
# ---------------------------------------------------------------------------------------------
CASES = {
    "47x47_two_chunks_scalar_loads": ((2, 3, 3, 47, 47), ("+w", "-h", None)),
    "64x64_two_chunks_quads": ((2, 2, 3, 64, 64), ("+w", "-h", None)),
    "7x9_partial_chunk": ((1, 2, 2, 7, 9), ("+h", "-w")),
    "one_scalar_40x40": ((2, 2, 1, 40, 40), (None,)),
    "two_scalars_of_four_32x32": ((1, 2, 4, 32, 32), (None, "-w", None, "+h")),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("y_transform", TRANSFORMS, ids=str)
@pytest.mark.parametrize("use_mask", [True, False])
def test_every_channel_equals_the_scalar_kernel_in_place(case, y_transform, use_mask):
    shape, axes = CASES[case]
    ds = vector_dataset(axes, y_transform)
    assert len({(ds.y_scale[c], ds.trans_min[c], ds.trans_max[c]) for c in range(ds.Cy)}) == ds.Cy        # constants of its own per channel
    y, yp, mask = _inputs(shape, 3)
    y_d, view, m_d = torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)), torch.from_numpy(mask).to(DEV)
    K = 8
    rep = U.VectorEvalReport(ds, points_per_bin=K, seed=5, device=DEV)
    rep.add(y_d, view, m_d, use_mask)
    assert rep.last_copies == 0 and rep.last_pointers[0] == view.data_ptr() and (not view.is_contiguous() or 1 in shape[:2])
    r = rep.result()
    assert r["axes"] == ds.axes and len(r["channels"]) == ds.Cy and (r["vector"] is None) == (case == "one_scalar_40x40")
    if np.prod(shape[:2]) * shape[3] * shape[4] >= 4000:
        assert all((ch["gt_bin_count"] > K).any() for ch in r["channels"])                               # the reservoir replaces
    _check_channels_equal_the_scalar_kernel(ds, rep, r, y_d, view, m_d, use_mask, K)
    n = int((mask != 0).sum()) if use_mask else int(np.prod(shape)) // shape[2]
    assert all(ch["n"] == n for ch in r["channels"]) and (r["vector"] is None or r["vector"]["n"] == n)


# 4096 bins and 1000 edges (-8 + i / 64: exact in binary): 3 * 4096 + 3 * 1001 = 15 291 counters fit the 15 360 of the scalar entry's
# LDS budget; the vector entry adds its speed and direction counters at every Cy, 15 291 + 3 * 4096 + 72, and counts in global memory.
ONE_CHANNEL = dict(hist_bins=4096, scatter_range=(-8.0, -8.0 + 999 / 64), scatter_bin_width=1 / 64)


@pytest.mark.parametrize("shape", [(2, 3, 1, 47, 47), (2, 2, 1, 64, 64)], ids=["47x47_scalar_loads", "64x64_quads"])
@pytest.mark.parametrize("use_mask", [True, False])
def test_one_channel_on_global_counters_equals_the_scalar_entry_on_lds_counters(shape, use_mask):
    """One tensor through uclstm_eval_stats (LDS counters) and, as Cy = 1, through uclstm_eval_stats_vec (global counters): the two
    entries run the LDS and the global instantiation of one kernel, and everything that does not depend on block arrival is equal."""
    ds = vector_dataset((None,), "asinh")
    y, yp, mask = _inputs(shape, 11)
    y_d, view, m_d = torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)), torch.from_numpy(mask).to(DEV)
    K = 8
    vec = U.VectorEvalReport(ds, points_per_bin=K, seed=5, device=DEV, **ONE_CHANNEL)
    sca = U.EvalReport(_One(ds, 0), points_per_bin=K, seed=5, device=DEV, **ONE_CHANNEL)
    words = 3 * 4096 + 3 * (len(sca.scatter_edges) + 1)
    assert len(vec.scatter_edges[0]) == len(sca.scatter_edges) == 1000 and vec.pair is None
    assert words == 15291 <= 15 * 1024 < words + 3 * 4096 + vec.dir_bins
    assert (shape[3] * shape[4] % 4 == 0) == (shape[3] == 64)                  # the 16-byte loader at 64 x 64 only
    vec.add(y_d, view, m_d, use_mask)
    sca.add(y_d, view, m_d, use_mask)
    assert vec.last_copies == 0 == sca.last_copies and vec.last_pointers == sca.last_pointers
    assert _bits(vec._tables[0][0][:, 0]) == _bits(sca._tables[0][0]), "table rows"
    assert torch.equal(vec._hist[0], sca._hist) and torch.equal(vec._dig[0], sca._dig), "counts"
    rv, rs = vec.result(), sca.result()
    assert rv["vector"] is None and len(rv["channels"]) == 1
    n = int((mask != 0).sum()) if use_mask else int(np.prod(shape))
    for r in (rv["channels"][0], rs):
        cnt = r["gt_bin_count"]
        assert cnt.sum() == n == r["n"]
        assert np.array_equal(np.bincount(r["scatter_bin"], minlength=len(cnt)), np.minimum(cnt, K)), "scatter fill"


def test_the_two_entry_points_share_no_state():
    """Scalar entry, vector entry with a pair, scalar entry again, in one process on tensors of one shape: the scalar entry reads
    [2,3,2,40,40] as one plane of 3200 elements, the vector entry as Cy = 2; the second scalar result is the first, bit for bit."""
    shape = (2, 3, 2, 40, 40)
    ds = vector_dataset(("+w", "-h"), "asinh")
    y, yp, _ = _inputs(shape, 13)
    y_d, view = torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp))

    def scalar():
        rep = U.EvalReport(_One(ds, 0), points_per_bin=8, seed=5, device=DEV)
        rep.add(y_d, view)
        assert rep.last_copies == 0 and rep._tables[0][0].shape[0] == 2 * 3 * 2                     # two chunks per frame
        return rep, rep.result()

    (rep_a, a) = scalar()
    vec = U.VectorEvalReport(ds, points_per_bin=8, seed=5, min_speed=MIN_SPEED, device=DEV)
    vec.add(y_d, view)
    v = vec.result()
    assert v["vector"] is not None and v["vector"]["n"] == 2 * 3 * 40 * 40 and len(v["channels"]) == 2
    (rep_b, b) = scalar()
    assert _bits(rep_a._tables[0][0]) == _bits(rep_b._tables[0][0])
    assert torch.equal(rep_a._hist, rep_b._hist) and torch.equal(rep_a._dig, rep_b._dig)
    _same(a, b, "scalar report")


# ---------------------------------------------------------------------------------------------
# inputs in polar form, and the f64 oracle
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _polar(axes, y_transform, shape, seed, anti=False):
    """Speeds of target and prediction from [0, 0.4] U [0.6, 9] m/s, the prediction's angle within 120 degrees of the target's (or
    opposite to it: anti), normalised through the forward transform.  Returns the dataset, y, y_pred, mask (f32 numpy)."""
    ds = vector_dataset(axes, y_transform)
    rng = np.random.default_rng(seed)
    B, T, Cy, H, W = shape
    plane = (B, T, H, W)

    def speeds():
        return np.where(rng.random(plane) < 0.25, rng.uniform(0.0, 0.4, plane), rng.uniform(0.6, 9.0, plane))

    sg, sp = speeds(), speeds()
    tg = rng.uniform(-np.pi, np.pi, plane)
    tp = tg + (np.pi if anti else np.radians(rng.uniform(-120.0, 120.0, plane)))
    raw_g, raw_p = rng.normal(0.0, 1.2, shape), rng.normal(0.0, 1.2, shape)
    w, h = ds.w_channel, ds.h_channel
    raw_g[:, :, w], raw_g[:, :, h] = sign(axes[w]) * sg * np.cos(tg), sign(axes[h]) * sg * np.sin(tg)
    raw_p[:, :, w], raw_p[:, :, h] = sign(axes[w]) * sp * np.cos(tp), sign(axes[h]) * sp * np.sin(tp)
    y, yp = VC.normalise64(raw_g, ds).astype(np.float32), VC.normalise64(raw_p, ds).astype(np.float32)
    mask = (rng.random((B, T, 1, H, W)) > 0.3).astype(np.float32)
    return ds, y, yp, mask


def _oracle(ds, y, yp, mask, use_mask, anti=False):
    """f64 (s_g, s_p, ds, epe, dtheta, valid, counted) from the dataset's own f32 denormalize, with the host-side guards."""
    gt, pr = ds.denormalize(y), ds.denormalize(yp)
    assert gt.dtype == np.float32 and pr.dtype == np.float32
    sg, sp, dsp, epe, th = vector_quantities(ds, gt, pr)
    valid = mask[:, :, 0] != 0 if use_mask else np.ones(sg.shape, dtype=bool)
    for s in (sg, sp):
        assert not np.any(valid & (np.abs(s - MIN_SPEED) <= DELTA)), "a valid pixel's speed lies within DELTA of min_speed"
    counted = valid & (sg >= MIN_SPEED) & (sp >= MIN_SPEED)
    if anti:
        assert np.all(np.abs(th[counted]) > 170.0)
    else:
        assert not np.any(np.abs(th[counted]) > 170.0), "a counted pixel's direction error can wrap"
    assert 0 < counted.sum() < valid.sum()
    return sg, sp, dsp, epe, th, valid, counted


def _near_edges(x, edges, delta):
    srt = np.sort(x)
    return np.searchsorted(srt, edges + delta, side="right") - np.searchsorted(srt, edges - delta, side="left")


def _check_hist(name, got, x, bins, rng_, delta, circular=False, max_share=0.01):
    """The rule of tests/test_gpu_eval_report.py::_check_hist: a count may differ from numpy's on the f64 values by the number of
    f64 values within delta of one of the bin's edges; circular: -180 and 180 are one edge (a value may land on either side)."""
    want, edges = np.histogram(x, bins, rng_)
    ne = _near_edges(x, edges, delta)
    if circular:
        ne[0] = ne[-1] = ne[0] + ne[-1]
    near = ne[:-1] + ne[1:]
    diff = np.abs(got.astype(np.int64) - want)
    share = ne.sum() / max(x.size, 1)
    print(f"[vector_report hist] {name}: bins that differ {int((diff > 0).sum())}, largest difference {int(diff.max())}, "
          f"values within {delta} of an edge {100 * share:.3f} %, counted {int(got.sum())} of {x.size}")
    assert max_share is None or share <= max_share, (name, share)
    assert np.all(diff <= near), (name, np.nonzero(diff > near)[0], diff[diff > near], near[diff > near])
    assert abs(int(got.sum()) - int(want.sum())) <= ne[0] + ne[-1], (name, int(got.sum()), int(want.sum()))


def _check_vector_hists(v, sg, sp, epe, th, valid, counted, bins, speed_hi, epe_hi, dir_bins, max_share=0.01):
    _check_hist("speed gt", v["hist_speed_gt"], sg[valid], bins, (0.0, speed_hi), DELTA, max_share=max_share)
    _check_hist("speed pred", v["hist_speed_pred"], sp[valid], bins, (0.0, speed_hi), DELTA, max_share=max_share)
    _check_hist("epe", v["hist_epe"], epe[valid], bins, (0.0, epe_hi), DELTA, max_share=max_share)
    _check_hist("direction", v["hist_dir"], th[counted], dir_bins, (-180.0, 180.0), DTHETA, circular=True, max_share=max_share)


POLAR_SHAPE = (2, 3, 3, 47, 47)
AXES = ("+w", "-h", None)


# ---------------------------------------------------------------------------------------------
# 2. the global-counter path
# ---------------------------------------------------------------------------------------------
def test_counters_beyond_the_lds_budget_use_the_global_path():
    shape = (1, 2, 3, 47, 47)
    ds, y, yp, mask = _polar(AXES, "asinh", shape, 31)
    kw = dict(hist_bins=4096, scatter_range=(-8.0, 8.0), scatter_bin_width=0.0008)
    K = 3
    rep = U.VectorEvalReport(ds, points_per_bin=K, min_speed=MIN_SPEED, device=DEV, **kw)
    n_edges = len(rep.scatter_edges[0])
    assert n_edges >= 20000 and (3 * (3 * 4096 + 3 * (n_edges + 1)) + 3 * 4096 + 72) * 4 > 60 * 1024
    assert (3 * 4096 + 3 * (n_edges + 1)) * 4 > 60 * 1024                     # the scalar kernel takes its global path too
    y_d, view, m_d = torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)), torch.from_numpy(mask).to(DEV)
    rep.add(y_d, view, m_d, True)
    r = rep.result()
    _check_channels_equal_the_scalar_kernel(ds, rep, r, y_d, view, m_d, True, K, pool=False, **kw)
    sg, sp, dsp, epe, th, valid, counted = _oracle(ds, y, yp, mask, True)
    v = r["vector"]
    assert v["n"] == valid.sum() and v["n_dir"] == counted.sum()
    assert _rel(v["epe_mean"], epe[valid].mean()) <= 1e-5 and _rel(v["speed_mae"], np.abs(dsp[valid]).mean()) <= 1e-5
    _check_vector_hists(v, sg, sp, epe, th, valid, counted, 4096, rep.speed_range[1], rep.epe_range[1], 72, max_share=None)


# ---------------------------------------------------------------------------------------------
# 3. vector sums, 4. vector histograms, 6. gating
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y_transform", TRANSFORMS, ids=str)
@pytest.mark.parametrize("use_mask", [True, False])
def test_vector_sums_and_histograms_against_f64_numpy(y_transform, use_mask):
    ds, y, yp, mask = _polar(AXES, y_transform, POLAR_SHAPE, 41)
    sg, sp, dsp, epe, th, valid, counted = _oracle(ds, y, yp, mask, use_mask)
    rep = U.VectorEvalReport(ds, min_speed=MIN_SPEED, device=DEV)
    view = _as_model_output(torch.from_numpy(yp))
    rep.add(torch.from_numpy(y).to(DEV), view, torch.from_numpy(mask).to(DEV), use_mask)
    assert rep.last_copies == 0 and rep.last_pointers[0] == view.data_ptr()
    v = rep.result()["vector"]
    tag = f"[vector_report sums] {y_transform}, mask {use_mask}:"
    # counts: exact (no valid speed within DELTA of min_speed, asserted by the oracle)
    assert v["n"] == valid.sum() and v["n_dir"] == counted.sum()
    w, wd = valid.astype(np.float64), counted.astype(np.float64)
    cols = {1: np.abs(dsp), 2: dsp * dsp, 3: dsp, 4: sg, 5: sp, 6: epe, 7: epe * epe}
    ang = {9: np.abs(th), 10: th, 11: th * th}
    ps = v["per_sequence"]
    assert ps.shape == POLAR_SHAPE[:2] + (16,)
    for name, axes_ in (("global", (0, 1, 2, 3)), ("per time step", (0, 2, 3)), ("per frame", (2, 3))):
        got = ps.sum(axis=tuple(a for a in axes_ if a < 2)) if name != "per frame" else ps
        n_, nd_ = w.sum(axis=axes_), wd.sum(axis=axes_)
        assert np.array_equal(got[..., 0], n_) and np.array_equal(got[..., 8], nd_)
        mag = (np.abs(dsp) * w).sum(axis=axes_)
        worst = {k: _rel(got[..., k], (x * w).sum(axis=axes_), scale=mag if k == 3 else None) for k, x in cols.items()}
        print(f"{tag} {name}: worst relative difference of the sums (|ds|, ds^2, ds, s_g, s_p, epe, epe^2) {[f'{e:.1e}' for e in worst.values()]}")
        assert max(worst.values()) <= 1e-5, (name, worst)
        over = {k: float(np.max(np.abs(got[..., k] - (x * wd).sum(axis=axes_)) / np.maximum(nd_ * DTHETA * (360.0 if k == 11 else 1.0), 1e-300)))
                for k, x in ang.items()}
        print(f"{tag} {name}: direction sums (|dth|, dth, dth^2), error as a share of n_dir * DTHETA (* 360 for dth^2) {[f'{e:.1e}' for e in over.values()]}")
        assert max(over.values()) <= 1.0, (name, over)
    # the figures of the report are those sums
    n, nd = valid.sum(), counted.sum()
    fig = {"speed_mae": np.abs(dsp[valid]).mean(), "speed_rmse": math.sqrt((dsp[valid] ** 2).mean()), "gt_speed_mean": sg[valid].mean(),
           "pred_speed_mean": sp[valid].mean(), "epe_mean": epe[valid].mean(), "epe_rmse": math.sqrt((epe[valid] ** 2).mean())}
    for k, want in fig.items():
        print(f"{tag} {k}: device {v[k]!r} host {float(want)!r} rel {_rel(v[k], want):.2e}")
        assert _rel(v[k], want) <= 1e-5, k
    assert _rel(v["speed_bias"], dsp[valid].mean(), scale=fig["speed_mae"]) <= 1e-5
    assert abs(v["epe_max"] - epe[valid].max()) <= DELTA
    for k, want in (("dir_mae", np.abs(th[counted]).mean()), ("dir_bias", th[counted].mean())):
        print(f"{tag} {k}: device {v[k]!r} host {float(want)!r} difference {v[k] - want:+.2e} degrees")
        assert abs(v[k] - want) <= DTHETA, k
    assert np.array_equal(v["per_timestep"]["n"], w.sum(axis=(0, 2, 3)))
    assert _rel(v["per_timestep"]["epe_mean"], (epe * w).sum(axis=(0, 2, 3)) / w.sum(axis=(0, 2, 3))) <= 1e-5
    assert np.all(np.abs(v["per_timestep"]["dir_mae"] - (np.abs(th) * wd).sum(axis=(0, 2, 3)) / wd.sum(axis=(0, 2, 3))) <= DTHETA)
    # 4. histograms
    assert np.array_equal(v["speed_edges"], np.linspace(0.0, 7.5, 101)) and np.array_equal(v["epe_edges"], np.linspace(0.0, 3.0, 101))
    _check_vector_hists(v, sg, sp, epe, th, valid, counted, 100, 7.5, 3.0, 72)
    assert np.mean(sg[valid] > 7.5) > 0.03 and np.mean(epe[valid] > 3.0) > 0.03                          # the drop rule is exercised
    # 6. gating: a pixel with either speed below min_speed is in the speed and epe sums (above) but in no direction count
    assert v["hist_dir"].sum() == nd < n
    rep0 = U.VectorEvalReport(ds, min_speed=0.0, device=DEV)
    rep0.add(torch.from_numpy(y).to(DEV), view, torch.from_numpy(mask).to(DEV), use_mask)
    v0 = rep0.result()["vector"]
    assert v0["n_dir"] == v0["n"] == n and v0["hist_dir"].sum() == n
    assert v0["per_sequence"][..., :8].tobytes() == ps[..., :8].tobytes() and v0["per_sequence"][..., 12:].tobytes() == ps[..., 12:].tobytes()


def test_anti_parallel_pairs_land_at_either_end_of_the_direction_histogram():
    ds, y, yp, mask = _polar(AXES, "asinh", POLAR_SHAPE, 43, anti=True)
    sg, sp, dsp, epe, th, valid, counted = _oracle(ds, y, yp, mask, True, anti=True)
    rep = U.VectorEvalReport(ds, min_speed=MIN_SPEED, device=DEV)
    rep.add(torch.from_numpy(y).to(DEV), _as_model_output(torch.from_numpy(yp)), torch.from_numpy(mask).to(DEV), True)
    v = rep.result()["vector"]
    assert v["n_dir"] == counted.sum()
    print(f"[vector_report sums] anti-parallel: dir_mae device {v['dir_mae']!r} host {float(np.abs(th[counted]).mean())!r}")
    assert abs(v["dir_mae"] - np.abs(th[counted]).mean()) <= DTHETA
    assert v["hist_dir"].sum() == counted.sum() and v["hist_dir"][1:-1].sum() == 0
    _check_hist("direction, anti-parallel", v["hist_dir"], th[counted], 72, (-180.0, 180.0), DTHETA, circular=True, max_share=None)


# ---------------------------------------------------------------------------------------------
# 5. the sign convention on a constructed field
# ---------------------------------------------------------------------------------------------
def _constant_field(axes, g_ab, p_ab, shape=(1, 2, 16, 16)):
    """Target and prediction constant in the IMAGE frame (a along +column, b along +row), stored under `axes`."""
    ds = vector_dataset(axes, None)
    B, T, H, W = shape
    raw = np.zeros((2, B, T, len(axes), H, W))
    for k, (a, b) in enumerate((g_ab, p_ab)):
        if ds.w_channel is not None:
            raw[k][:, :, ds.w_channel] = sign(axes[ds.w_channel]) * a
        if ds.h_channel is not None:
            raw[k][:, :, ds.h_channel] = sign(axes[ds.h_channel]) * b
    y, yp = (torch.from_numpy(VC.normalise64(r, ds).astype(np.float32)).to(DEV) for r in raw)
    rep = U.VectorEvalReport(ds, dir_bins=8, min_speed=MIN_SPEED, device=DEV)
    rep.add(y, yp)
    return rep, rep.result()


def test_sign_convention_on_a_constructed_field():
    g, p = (1.0, 0.0), (math.cos(math.radians(30.0)), math.sin(math.radians(30.0)))       # turned by +30 degrees towards +row
    n = 2 * 16 * 16
    for axes in (("+w", "+h"), ("+w", "-h"), ("-w", "+h"), ("-h", "+w")):
        _, r = _constant_field(axes, g, p)
        v = r["vector"]
        print(f"[vector_report sign] {axes}: dir_bias {v['dir_bias']!r} dir_mae {v['dir_mae']!r} epe_mean {v['epe_mean']!r} speed_mae {v['speed_mae']!r}")
        assert v["n"] == v["n_dir"] == n
        assert abs(v["dir_bias"] - 30.0) <= DTHETA and abs(v["dir_mae"] - 30.0) <= DTHETA and v["dir_std"] <= DTHETA
        assert abs(v["epe_mean"] - 2.0 * math.sin(math.radians(15.0))) <= DELTA and v["speed_mae"] <= DELTA
        assert v["hist_dir"][4] == n and v["hist_dir"].sum() == n                        # 8 bins of 45 degrees: [0, 45)
    _, r = _constant_field(("+w", "-h"), p, g)                                           # prediction and target swapped
    v = r["vector"]
    assert abs(v["dir_bias"] + 30.0) <= DTHETA and abs(v["dir_mae"] - 30.0) <= DTHETA and v["hist_dir"][3] == n
    # one horizontal channel only: no vector part, and its buffers do not exist, so the kernel was given none to touch
    rep, r = _constant_field(("+w", None), g, p)
    assert r["vector"] is None and rep._vhist is None and rep._dir is None and rep._tables[0][1] is None
    assert len(r["channels"]) == 2 and r["channels"][0]["n"] == n and abs(r["channels"][0]["mae"] - (1.0 - p[0])) <= DELTA


# ---------------------------------------------------------------------------------------------
# 7. reproducibility and accumulation
# ---------------------------------------------------------------------------------------------
def _same(u, v, key):
    if isinstance(u, dict):
        assert set(u) == set(v), key
        for k in u:
            if k not in ("scatter_gt", "scatter_pred"):
                _same(u[k], v[k], f"{key}.{k}")
            else:
                assert len(u[k]) == len(v[k]), f"{key}.{k}"
    elif isinstance(u, (list, tuple)):
        assert len(u) == len(v), key
        for i, (a, b) in enumerate(zip(u, v)):
            _same(a, b, f"{key}[{i}]")
    elif isinstance(u, np.ndarray):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), key
    elif u is None or isinstance(u, str):
        assert u == v, key
    else:
        assert np.float64(u).tobytes() == np.float64(v).tobytes(), key


def test_two_runs_are_bitwise_equal_and_two_adds_equal_one():
    shape = (4, 3, 3, 47, 47)
    ds, y, yp, mask = _polar(AXES, "asinh", shape, 47)

    def run(pieces):
        rep = U.VectorEvalReport(ds, points_per_bin=20, min_speed=MIN_SPEED, device=DEV)
        for s in pieces:
            rep.add(torch.from_numpy(y[s]).to(DEV), _as_model_output(torch.from_numpy(yp[s])), torch.from_numpy(mask[s]).to(DEV), True)
        return rep, rep.result()

    halves = (slice(0, 1), slice(1, 4))
    (_, a), (_, b), (rep, one) = run(halves), run(halves), run((slice(0, 4),))
    _same(a, b, "report")
    # two add() calls against one on the concatenation: counts, histograms, per-sequence rows
    for c in range(3):
        for k in ("n", "hist_gt", "hist_pred", "hist_err", "gt_bin_count", "per_sequence"):
            _same(a["channels"][c][k], one["channels"][c][k], f"channels[{c}].{k}")
    for k in ("n", "n_dir", "hist_speed_gt", "hist_speed_pred", "hist_epe", "hist_dir", "per_sequence"):
        _same(a["vector"][k], one["vector"][k], f"vector.{k}")
    with pytest.raises(U.UclstmError):
        rep.add(torch.from_numpy(y[:, :2]).to(DEV), torch.from_numpy(yp[:, :2]).to(DEV))                 # T = 2 after T = 3


# ---------------------------------------------------------------------------------------------
# 8. evaluate_vector_report and the tool
# ---------------------------------------------------------------------------------------------
def _wind_npz(path, N, T=3, S=32, seed=0):
    rng = np.random.default_rng(seed)
    X = (rng.random((N, T, 2, S, S)) * 30).astype(np.float32)
    X[X < 6] = 0.0
    base = np.tanh(X[:, :, :1] / 15.0 - 1.0).astype(np.float32)
    Y = np.concatenate([base * 9.0 + rng.standard_normal(base.shape).astype(np.float32), np.roll(base, 3, axis=-1) * -8.0, base * 1.5],
                       axis=2).astype(np.float32)
    np.savez(path, X=X, Y=Y)


def _model():
    torch.manual_seed(0)
    return U.TemporalUNetDualView(1, 3, base_ch=16, lstm_layers=1, use_skip_lstm=True, use_attention=False)


def test_evaluate_vector_report_returns_what_evaluate_returns(tmp_path):
    """The first four values against a separate evaluate() pass, to evaluate()'s own run-to-run freedom as
    tests/test_gpu_eval_report.py states it: the loss is rounded to f32 per batch (2^-23 relative), the metric sums <= 1e-12."""
    _wind_npz(tmp_path / "wind.npz", 6)
    dev = torch.device(DEV)
    model = _model().to(DEV)
    for tie, tta in ((False, None), (False, "flips"), (True, "d4")):
        ds = U.VectorNPZDataset(str(tmp_path / "wind.npz"), AXES, tie_horizontal=tie, lower_percentile=0.5, upper_percentile=99.5)
        loader = U.DeviceSequenceLoader(ds, 2)
        ev = U.evaluate(model, loader, dev, ds, use_mask=True, per_channel=True, tta=tta)
        out = U.evaluate_vector_report(model, loader, dev, ds, use_mask=True, tta=tta, points_per_bin=10)
        assert len(out) == 5
        rep = out[4]
        print(f"[vector_report evaluate] tie {tie} tta {tta}: evaluate {ev[:4]}, evaluate_vector_report {out[:4]}, "
              f"channel mae {[ch['mae'] for ch in rep['channels']]}, vector epe {rep['vector']['epe_mean']}")
        assert abs(out[0] - ev[0]) <= 2.0 ** -23 * abs(ev[0]), (out[0], ev[0])
        assert _rel(out[1], ev[1]) <= 1e-12 and _rel(out[2], ev[2]) <= 1e-12 and _rel(out[3], ev[3], scale=ev[1]) <= 1e-12, (out[:4], ev[:4])
        for c in range(3):
            assert _rel(rep["channels"][c]["mae"], ev[4]["mae"][c]) <= 1e-5 and _rel(rep["channels"][c]["rmse"], ev[4]["rmse"][c]) <= 1e-5
            assert rep["channels"][c]["per_sequence"].shape == (6, 3, 4)
        assert rep["axes"] == AXES and rep["vector"]["per_sequence"].shape == (6, 3, 16)
        assert rep["vector"]["n"] == rep["channels"][0]["n"] and math.isfinite(rep["vector"]["dir_mae"])


def test_tool_writes_the_vector_report(tmp_path):
    npz, ckpt, out = tmp_path / "wind.npz", tmp_path / "model.pt", tmp_path / "report.npz"
    _wind_npz(npz, 10)
    model = _model()
    torch.save({"config": {"type": "custom", "base_ch": 16, "use_skip_lstm": True, "use_attention": False}, "model_state": model.state_dict()}, ckpt)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_report.py"), "--checkpoint", str(ckpt), "--npz", str(npz), "--axes", "+w,-h,none",
           "--tie-horizontal", "--batch", "2", "--use-mask", "--out", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for line in ("Speed MAE:", "Endpoint Error:", "Direction MAE:", "Channel 2 (None):"):
        assert line in p.stdout, p.stdout
    ds = U.VectorNPZDataset(str(npz), AXES, tie_horizontal=True)
    n_train = int(0.8 * len(ds))
    _, val = torch.utils.data.random_split(ds, [n_train, len(ds) - n_train], generator=torch.Generator().manual_seed(42))
    want = U.evaluate(model.to(DEV), U.DeviceSequenceLoader(val, 2), torch.device(DEV), ds, use_mask=True, per_channel=True)
    with np.load(out, allow_pickle=False) as z:
        got = {k: z[k] for k in z.files}
    assert list(got["axes"]) == ["+w", "-h", "none"]
    for c in range(3):
        assert _rel(got[f"ch{c}_mae"], want[4]["mae"][c]) <= 1e-5 and got[f"ch{c}_hist_gt"].shape == (100,)
    for k in ("n", "speed_mae", "speed_rmse", "speed_bias", "gt_speed_mean", "pred_speed_mean", "epe_mean", "epe_rmse", "epe_max", "n_dir", "dir_mae",
              "dir_bias", "dir_std", "per_timestep_speed_mae", "per_timestep_epe_mean", "per_timestep_dir_mae", "per_timestep_n", "per_sequence",
              "hist_speed_gt", "hist_speed_pred", "hist_epe", "hist_dir", "speed_edges", "epe_edges", "dir_edges"):
        assert f"vector_{k}" in got, k
    assert got["vector_per_sequence"].shape == (len(val), 3, 16) and got["vector_hist_dir"].shape == (72,)
