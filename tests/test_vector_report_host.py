"""CPU-only tests of the vector evaluation report: the C ABI of uclstm_eval_stats_vec (symbol, descriptor mirror, argument contract
-- nothing is launched), VectorEvalReport.reduce_vector against numpy in f64 on hand-built tables, the documented defaults, and
the refusals on both sides (EvalReport keeps refusing a vector dataset, VectorEvalReport refuses a scalar one)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L

from vector_report_cases import vector_dataset

VROW = 16


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def _desc(over=()):
    """A descriptor that passes validation (its pointers are garbage: a call that accepted it would launch)."""
    d = L.EvalVecDesc()
    junk = 0x1000
    d.y_pred, d.y, d.mask, d.table, d.hist, d.dig_count, d.scatter, d.vtable, d.vhist, d.dir_hist = (junk,) * 10
    d.pred_stride_b, d.pred_stride_t, d.y_stride_b, d.y_stride_t, d.mask_stride_b, d.mask_stride_t = 3072, 768, 3072, 768, 1024, 256
    d.B, d.T, d.Cy, d.transform, d.HW = 2, 4, 3, L.EVAL_ASINH, 256
    for c in range(L.VEC_MAX):
        d.consts[c] = L.TargetConsts(-8.0, 9.0, 2.0 + c, -2.0, 2.2)
        d.hist_lo[c], d.hist_hi[c], d.err_lo[c], d.err_hi[c], d.dig_lo[c], d.dig_w[c] = -7.5, 7.5, -3.0, 3.0, -8.0, 0.05
    d.bins, d.n_edges, d.K, d.dir_bins, d.seed = 100, 321, 1000, 72, 0
    d.w_chan, d.h_chan, d.w_sign, d.h_sign = 0, 1, 1, -1
    d.speed_hi, d.epe_hi, d.min_speed = 7.5, 3.0, 0.5
    for k, v in dict(over).items():
        if isinstance(k, tuple):                                    # (array field, channel)
            getattr(d, k[0])[k[1]] = v
        else:
            setattr(d, k, v)
    return d


def test_eval_stats_vec_is_in_the_header_the_binding_and_the_library():
    hdr = open(L.HEADER_PATH).read()
    raw = C.CDLL(L.LIB_PATH)
    sym = "uclstm_eval_stats_vec"
    assert re.search(r"\b%s\s*\(" % sym, hdr)
    assert sym in L._PROTOS and sym in L.header_symbols() and hasattr(raw, sym)
    assert sym not in L.F16_TWINS and not hasattr(raw, sym + "_f16")
    assert int(re.search(r"#define UCLSTM_EVAL_VROW\s+(\d+)", hdr).group(1)) == L.EVAL_VROW == U.VectorEvalReport.VROW == VROW
    assert int(re.search(r"#define UCLSTM_VEC_MAX\s+(\d+)", hdr).group(1)) == L.VEC_MAX == 4
    # the ctypes mirror has the header's field list, in order, arrays of UCLSTM_VEC_MAX where the header has them
    body = re.search(r"typedef struct \{([^}]*)\}\s*uclstm_eval_vec_desc;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, arrays = [], set()
    for decl in body.split(";"):
        for part in decl.strip().split(","):
            part = part.strip()
            if part:
                name = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part.split("[")[0])[-1]
                names.append(name)
                if "[UCLSTM_VEC_MAX]" in part:
                    arrays.add(name)
    assert names == [f[0] for f in L.EvalVecDesc._fields_]
    assert arrays == {f[0] for f in L.EvalVecDesc._fields_ if issubclass(f[1], C.Array)}
    assert all(f[1]._length_ == L.VEC_MAX for f in L.EvalVecDesc._fields_ if issubclass(f[1], C.Array))
    # 9 words of tensors, B T Cy transform, HW, consts, six f64 arrays, four ints, seed, four ints, three doubles, seven pointers
    assert C.sizeof(L.EvalVecDesc) == 9 * 8 + 16 + 8 + 4 * 20 + 6 * 4 * 8 + 16 + 8 + 16 + 3 * 8 + 7 * 8
    assert C.sizeof(L.TargetConsts) == 20


BAD = {
    "null y_pred": dict(y_pred=None), "null y": dict(y=None), "null table": dict(table=None), "null hist": dict(hist=None),
    "null dig_count": dict(dig_count=None), "null scatter with K > 0": dict(scatter=None),
    "HW = 0": dict(HW=0), "HW < 0": dict(HW=-4), "B = 0": dict(B=0), "T < 0": dict(T=-1),
    "bins = 0": dict(bins=0), "bins = 4097": dict(bins=4097),
    "hist hi == lo, channel 0": {("hist_hi", 0): -7.5}, "hist hi < lo, channel 2": {("hist_hi", 2): -8.0},
    "err hi <= lo, channel 1": {("err_hi", 1): -3.0},
    "w = 0, channel 2": {("dig_w", 2): 0.0}, "w < 0, channel 0": {("dig_w", 0): -0.05}, "w nan, channel 1": {("dig_w", 1): float("nan")},
    "dig_lo nan, channel 2": {("dig_lo", 2): float("nan")},
    "y_scale = 0, channel 1": {("consts", 1): L.TargetConsts(-8.0, 9.0, 0.0, -2.0, 2.2)},
    "n_edges = 1": dict(n_edges=1), "n_edges = 65537": dict(n_edges=65537),
    "K < 0": dict(K=-1), "transform 3": dict(transform=3), "transform -1": dict(transform=-1),
    "negative stride": dict(pred_stride_t=-256), "negative mask stride": dict(mask_stride_b=-4),
    "Cy = 0": dict(Cy=0), "Cy = 5": dict(Cy=5),
    "w_chan = Cy": dict(w_chan=3), "w_chan = -2": dict(w_chan=-2), "h_chan = Cy": dict(h_chan=3), "h_chan = -2": dict(h_chan=-2),
    "w_chan == h_chan": dict(w_chan=1, h_chan=1),
    "w_sign = 0": dict(w_sign=0), "h_sign = 2": dict(h_sign=2),
    "speed_hi = 0": dict(speed_hi=0.0), "speed_hi nan": dict(speed_hi=float("nan")), "epe_hi < 0": dict(epe_hi=-1.0),
    "min_speed < 0": dict(min_speed=-0.1), "min_speed nan": dict(min_speed=float("nan")),
    "dir_bins = 0": dict(dir_bins=0), "dir_bins = 4097": dict(dir_bins=4097),
    "null vtable with a pair": dict(vtable=None), "null vhist with a pair": dict(vhist=None), "null dir_hist with a pair": dict(dir_hist=None),
    "2^31 elements": dict(B=1 << 14, T=1 << 4, Cy=2, HW=1 << 12), "beyond 2^31 elements": dict(B=1 << 20, T=1 << 10, HW=1 << 20),
    "2^31 only with Cy": dict(B=1 << 14, T=1 << 4, Cy=4, HW=1 << 11, w_chan=0, h_chan=1),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_eval_stats_vec_rejects_bad_arguments_before_any_launch(name):
    # no GPU here and the pointers are garbage: anything but an early UCLSTM_E_BADARG would be a launch error (-2) or a crash
    assert L.lib.uclstm_eval_stats_vec(C.byref(_desc(BAD[name])), None) == -1, name


def test_eval_stats_vec_rejects_a_null_descriptor():
    assert L.lib.uclstm_eval_stats_vec(None, None) == -1


# ---------------------------------------------------------------------------------------------
# the class: refusals, defaults
# ---------------------------------------------------------------------------------------------
class _Scalar:
    y_transform, y_scale, trans_min, trans_max = "asinh", 2.0, -2.0, 2.2


def test_each_report_refuses_the_other_kind_of_dataset():
    vec = vector_dataset(("+w", "-h", None))
    with pytest.raises(TypeError, match="EvalReport"):
        U.VectorEvalReport(_Scalar())
    with pytest.raises(TypeError, match="EvalReport"):
        U.evaluate_vector_report(None, [], "cpu", _Scalar())
    with pytest.raises(TypeError, match="vector"):
        U.EvalReport(vec, device="cpu")
    with pytest.raises(TypeError, match="vector"):
        U.evaluate_report(None, [], "cpu", vec)


def test_the_three_evaluation_functions_keep_their_parameter_lists():
    """One loop serves all three; what a caller passes, and in which order a wrong dataset is refused, is unchanged."""
    head = ["model", "loader", "device", "dataset_obj", "use_mask"]
    assert list(inspect.signature(U.evaluate).parameters) == head + ["per_channel", "tta", "loss"]
    assert list(inspect.signature(U.evaluate_report).parameters) == head + ["tta", "loss", "report_kwargs"]
    assert list(inspect.signature(U.evaluate_vector_report).parameters) == head + ["tta", "loss", "report_kwargs"]
    for fn in (U.evaluate, U.evaluate_report, U.evaluate_vector_report):
        sig = inspect.signature(fn).parameters
        assert sig["use_mask"].default is True and sig["tta"].default is None and sig["loss"].default is None
        assert all(sig[k].default is inspect.Parameter.empty for k in head[:4])
    assert inspect.signature(U.evaluate).parameters["per_channel"].default is False
    for fn in (U.evaluate_report, U.evaluate_vector_report):
        assert inspect.signature(fn).parameters["report_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the wrong dataset is refused before the loss is looked at (a bad `loss` alone is a TypeError that names it)
    vec = vector_dataset(("+w", "-h", None))
    with pytest.raises(TypeError, match="vector"):
        U.evaluate_report(None, [], "cpu", vec, loss="l2")
    with pytest.raises(TypeError, match="EvalReport"):
        U.evaluate_vector_report(None, [], "cpu", _Scalar(), loss="l2")
    with pytest.raises(TypeError, match="LossSpec"):
        U.evaluate_report(None, [], "cpu", _Scalar(), loss="l2")
    with pytest.raises(TypeError, match="LossSpec"):
        U.evaluate_vector_report(None, [], "cpu", vec, loss="l2")


def test_cpu_tensors_raise():
    rep = U.VectorEvalReport(vector_dataset(("+w", "-h", None)))
    y = torch.zeros(1, 2, 3, 4, 4)
    with pytest.raises(U.UclstmError):
        rep.add(y, y)
    with pytest.raises(U.UclstmError):
        rep.result()


def test_defaults_are_as_documented():
    sig = inspect.signature(U.VectorEvalReport.__init__).parameters
    want = dict(hist_bins=100, hist_range=(-7.5, 7.5), err_range=(-3.0, 3.0), scatter_range=(-8.0, 8.0), scatter_bin_width=0.05,
                points_per_bin=1000, speed_range=None, epe_range=None, dir_bins=72, min_speed=0.5, seed=0, device="cuda")
    assert {k: sig[k].default for k in want} == want and list(sig) == ["self", "dataset_obj"] + list(want)
    sig = inspect.signature(U.evaluate_vector_report).parameters
    assert list(sig)[:7] == ["model", "loader", "device", "dataset_obj", "use_mask", "tta", "loss"] and sig["use_mask"].default is True
    rep = U.VectorEvalReport(vector_dataset(("+w", "-h", None)))
    assert rep.speed_range == (0.0, 7.5) and rep.epe_range == (0.0, 3.0) and rep.pair == (0, 1)
    assert rep.hist_range == [(-7.5, 7.5)] * 3 and len(rep.scatter_edges) == 3
    assert all(np.array_equal(e, U.EvalReport.make_scatter_edges((-8.0, 8.0), 0.05)) for e in rep.scatter_edges)
    # per channel: the defaults look at the two horizontal channels only (here channels 2 and 0; channel 1 is the scalar)
    rep = U.VectorEvalReport(vector_dataset(("-h", None, "+w")), hist_range=[(-6.0, 4.0), (-30.0, 30.0), (-5.0, 5.5)],
                             err_range=[(-2.0, 1.0), (-9.0, 9.0), (-1.5, 1.75)], scatter_range=[(-8.0, 8.0), (-4.0, 12.0), (-8.0, 8.0)])
    assert rep.pair == (2, 0) and rep.speed_range == (0.0, 6.0) and rep.epe_range == (0.0, 2.0)
    assert rep.scatter_edges[1][0] == -4.0 and len({len(e) for e in rep.scatter_edges}) == 1
    rep = U.VectorEvalReport(vector_dataset(("+w", None)), speed_range=(0.0, 4.0))
    assert rep.pair is None and rep.speed_range == (0.0, 4.0)
    with pytest.raises(ValueError):
        U.VectorEvalReport(vector_dataset(("+w", "-h")), scatter_range=[(-8.0, 8.0), (-8.0, 9.0)])     # different edge counts
    with pytest.raises(ValueError):
        U.VectorEvalReport(vector_dataset(("+w", "-h")), hist_range=[(-1.0, 1.0)] * 3)
    with pytest.raises(ValueError):
        U.VectorEvalReport(vector_dataset(("+w", "-h")), min_speed=-1.0)


# ---------------------------------------------------------------------------------------------
# VectorEvalReport.reduce_vector
# ---------------------------------------------------------------------------------------------
def _vtables_numpy(ga, gb, pa, pb, valid, chunks, min_speed):
    """Rows as uclstm_eval_stats_vec defines them, from f64 image-frame components [B,T,H,W], the plane cut into `chunks` pieces."""
    B, T = ga.shape[:2]
    ga, gb, pa, pb, v = (a.reshape(B, T, chunks, -1) for a in (ga, gb, pa, pb, valid))
    sg, sp = np.hypot(ga, gb), np.hypot(pa, pb)
    ds, epe = sp - sg, np.hypot(pa - ga, pb - gb)
    th = np.degrees(np.arctan2(ga * pb - gb * pa, ga * pa + gb * pb))
    vd = v & (sg >= min_speed) & (sp >= min_speed)
    tab = np.zeros((B, T, chunks, VROW))
    for k, a in enumerate((np.ones_like(ds), np.abs(ds), ds * ds, ds, sg, sp, epe, epe * epe)):
        tab[..., k] = np.where(v, a, 0.0).sum(axis=-1)
    for k, a in enumerate((np.ones_like(th), np.abs(th), th, th * th)):
        tab[..., 8 + k] = np.where(vd, a, 0.0).sum(axis=-1)
    for k, a in enumerate((epe, sg, sp)):
        tab[..., 12 + k] = np.where(v, a, -np.inf).max(axis=-1)
    return tab, (sg, sp, ds, epe, th, v, vd)


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1e-300)), (a, b)


@pytest.mark.parametrize("use_mask", [False, True])
def test_reduce_vector_matches_numpy(use_mask):
    rng = np.random.default_rng(17)
    N, T, H, W = 5, 4, 12, 12
    ga, gb = rng.normal(0.5, 3.0, (N, T, H, W)), rng.normal(-0.3, 2.0, (N, T, H, W))
    grow = (1.0 + np.arange(T))[None, :, None, None] / T
    pa, pb = ga + rng.normal(0.1, 0.8, ga.shape) * grow, gb + rng.normal(0.0, 0.8, ga.shape) * grow
    valid = rng.random(ga.shape) > 0.35 if use_mask else np.ones(ga.shape, dtype=bool)
    if use_mask:
        valid[1, 2] = False                                          # a frame without one valid pixel
    parts = [_vtables_numpy(ga[s], gb[s], pa[s], pb[s], valid[s], 2, 0.5) for s in (slice(0, 3), slice(3, 5))]
    sg, sp, ds, epe, th, v, vd = (np.concatenate([p[1][k].reshape(-1, T, H * W) for p in parts]) for k in range(7))
    bins, dir_bins = 20, 72
    vhist = np.stack([np.histogram(sg[v], bins, (0.0, 7.5))[0], np.histogram(sp[v], bins, (0.0, 7.5))[0], np.histogram(epe[v], bins, (0.0, 3.0))[0]])
    dir_hist = np.histogram(th[vd], dir_bins, (-180.0, 180.0))[0]
    r = U.VectorEvalReport.reduce_vector([p[0] for p in parts], vhist.astype(np.uint64), dir_hist.astype(np.uint64),
                                         speed_range=(0.0, 7.5), epe_range=(0.0, 3.0))
    assert r["n"] == float(v.sum()) and r["n_dir"] == float(vd.sum()) and 0 < r["n_dir"] < r["n"]
    _close(r["speed_mae"], np.abs(ds[v]).mean())
    _close(r["speed_rmse"], np.sqrt((ds[v] ** 2).mean()))
    _close(r["speed_bias"], ds[v].mean())
    _close([r["gt_speed_mean"], r["pred_speed_mean"]], [sg[v].mean(), sp[v].mean()])
    _close([r["epe_mean"], r["epe_rmse"], r["epe_max"]], [epe[v].mean(), np.sqrt((epe[v] ** 2).mean()), epe[v].max()])
    _close(r["dir_mae"], np.abs(th[vd]).mean())
    _close(r["dir_bias"], th[vd].mean())
    _close(r["dir_std"], th[vd].std())
    pt = r["per_timestep"]
    for t in range(T):
        vt, vdt = v[:, t], vd[:, t]
        assert pt["n"][t] == vt.sum()
        _close(pt["speed_mae"][t], np.abs(ds[:, t][vt]).mean())
        _close(pt["epe_mean"][t], epe[:, t][vt].mean())
        _close(pt["dir_mae"][t], np.abs(th[:, t][vdt]).mean())
    ps = r["per_sequence"]
    assert ps.shape == (N, T, VROW) and len(U.VectorEvalReport.VSUMS) == VROW
    for i in range(N):
        for t in range(T):
            m, md = v[i, t], vd[i, t]
            assert ps[i, t, 0] == m.sum() and ps[i, t, 8] == md.sum() and ps[i, t, 15] == 0.0
            if m.any():
                _close(ps[i, t, [1, 2, 4, 5, 6, 7]], [np.abs(ds[i, t][m]).sum(), (ds[i, t][m] ** 2).sum(), sg[i, t][m].sum(), sp[i, t][m].sum(),
                                                      epe[i, t][m].sum(), (epe[i, t][m] ** 2).sum()])
                _close(ps[i, t, 12:15], [epe[i, t][m].max(), sg[i, t][m].max(), sp[i, t][m].max()])
                _close(ps[i, t, [9, 11]], [np.abs(th[i, t][md]).sum(), (th[i, t][md] ** 2).sum()])
            else:
                assert not ps[i, t, :12].any() and np.all(ps[i, t, 12:15] == -np.inf)
    for k, h in zip(("hist_speed_gt", "hist_speed_pred", "hist_epe"), vhist):
        assert r[k].dtype == np.int64 and np.array_equal(r[k], h)
    assert r["hist_dir"].dtype == np.int64 and np.array_equal(r["hist_dir"], dir_hist)
    assert np.array_equal(r["speed_edges"], np.histogram(sg[v], bins, (0.0, 7.5))[1])
    assert np.array_equal(r["epe_edges"], np.linspace(0.0, 3.0, bins + 1)) and np.array_equal(r["dir_edges"], np.linspace(-180, 180, dir_bins + 1))


def test_reduce_vector_of_nothing_valid_is_all_zero():
    tab = np.zeros((1, 2, 1, VROW))
    tab[..., 12:15] = -np.inf
    r = U.VectorEvalReport.reduce_vector([tab], np.zeros((3, 4), np.uint64), np.zeros(8, np.uint64), speed_range=(0, 1), epe_range=(0, 1))
    assert r["n"] == 0 and r["n_dir"] == 0
    assert r["speed_mae"] == r["speed_rmse"] == r["epe_mean"] == r["epe_max"] == r["dir_mae"] == r["dir_bias"] == r["dir_std"] == 0.0
    assert not r["per_timestep"]["dir_mae"].any() and not r["per_timestep"]["epe_mean"].any()
