"""CPU-only tests of the evaluation report: the C ABI of uclstm_eval_stats (symbols, argument contract -- nothing is launched),
EvalReport.reduce against the numpy formulas of train/get_metrics.py / test.py in f64, and the reference's bin constants."""
import ctypes as C
import inspect
import math
import re

import numpy as np
import pytest
import torch

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd.engine import EvalReport

ROW = 16


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def _desc(**over):
    """A descriptor that passes validation (its pointers are garbage: a call that accepted it would launch)."""
    d = L.EvalDesc()
    junk = 0x1000
    d.y_pred, d.y, d.mask, d.table, d.hist, d.dig_count, d.scatter = (junk,) * 7
    d.pred_stride_b, d.pred_stride_t, d.y_stride_b, d.y_stride_t, d.mask_stride_b, d.mask_stride_t = 1024, 256, 1024, 256, 1024, 256
    d.B, d.T, d.P = 2, 4, 256
    d.transform, d.y_scale, d.trans_min, d.trans_max = L.EVAL_ASINH, 2.0, -2.0, 2.2
    d.bins, d.n_edges = 100, 321
    d.hist_lo, d.hist_hi, d.err_lo, d.err_hi = -7.5, 7.5, -3.0, 3.0
    d.dig_lo, d.dig_w = -8.0, 0.05
    d.seed, d.K = 0, 1000
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_eval_stats_is_in_the_header_the_binding_and_the_library():
    hdr = open(L.HEADER_PATH).read()
    raw = C.CDLL(L.LIB_PATH)
    for sym in ("uclstm_eval_stats", "uclstm_eval_stats_rows"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in L._PROTOS and sym in L.header_symbols() and hasattr(raw, sym), sym
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16            # additive change
    assert len(L.F16_TWINS) == 29 and "uclstm_eval_stats" not in L.F16_TWINS
    assert int(re.search(r"#define UCLSTM_EVAL_ROW\s+(\d+)", hdr).group(1)) == L.EVAL_ROW == EvalReport.ROW == ROW
    # the ctypes mirror has the header's field list, in order
    body = re.search(r"typedef struct \{([^}]*)\}\s*uclstm_eval_desc;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", first)[-1]] + [r.strip().lstrip("*") for r in rest]
    assert names == [f[0] for f in L.EvalDesc._fields_]
    assert C.sizeof(L.EvalDesc) == 9 * 8 + 8 + 8 + 16 + 8 + 8 + 6 * 8 + 3 * 8 + 8 + 8


def test_eval_stats_rows_depend_on_the_plane_and_frame_count_only():
    rows = L.lib.uclstm_eval_stats_rows
    assert rows(64 * 64, 640) == 640 * rows(64 * 64, 1)
    assert rows(512 * 512, 1) >= 64                                     # a 512 x 512 frame is not one block
    assert rows(256 * 256, 12) >= 256                                   # B = 1, T = 12 still fills 256 compute units
    assert rows(1, 7) == 7 and rows(255, 3) == 3
    per_frame = [rows(p, 1) for p in (1, 1000, 4096, 4097, 65536)]
    assert per_frame == sorted(per_frame)
    for p, f in ((0, 4), (-1, 4), (16, 0), (16, -2), (1 << 31, 1)):
        assert rows(p, f) == -1


BAD = {
    "null y_pred": dict(y_pred=None), "null y": dict(y=None), "null table": dict(table=None), "null hist": dict(hist=None),
    "null dig_count": dict(dig_count=None), "null scatter with K > 0": dict(scatter=None),
    "P = 0": dict(P=0), "P < 0": dict(P=-4), "B = 0": dict(B=0), "T < 0": dict(T=-1),
    "bins = 0": dict(bins=0), "bins = 4097": dict(bins=4097),
    "hist hi == lo": dict(hist_hi=-7.5), "hist hi < lo": dict(hist_hi=-8.0), "err hi <= lo": dict(err_hi=-3.0),
    "w = 0": dict(dig_w=0.0), "w < 0": dict(dig_w=-0.05), "w nan": dict(dig_w=float("nan")),
    "n_edges = 1": dict(n_edges=1), "n_edges = 65537": dict(n_edges=65537),
    "K < 0": dict(K=-1), "transform 3": dict(transform=3), "transform -1": dict(transform=-1),
    "2^31 elements": dict(B=1 << 15, T=1 << 4, P=1 << 12), "beyond 2^31 elements": dict(B=1 << 20, T=1 << 10, P=1 << 20),
    "negative stride": dict(pred_stride_t=-256),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_eval_stats_rejects_bad_arguments_before_any_launch(name):
    # no GPU here and the pointers are garbage: anything but an early UCLSTM_E_BADARG would be a launch error (-2) or a crash
    assert L.lib.uclstm_eval_stats(C.byref(_desc(**BAD[name])), None) == -1, name


def test_eval_stats_rejects_a_null_descriptor():
    assert L.lib.uclstm_eval_stats(None, None) == -1


def test_cpu_tensors_raise():
    ds = _FakeDataset()
    rep = U.EvalReport(ds)
    y = torch.zeros(1, 2, 1, 4, 4)
    with pytest.raises(U.UclstmError):
        rep.add(y, y)
    with pytest.raises(U.UclstmError):
        rep.result()


# ---------------------------------------------------------------------------------------------
# constants of the reference
# ---------------------------------------------------------------------------------------------
class _FakeDataset:
    y_transform, y_scale, trans_min, trans_max = "asinh", 2.0, -2.0, 2.2


def test_defaults_and_edges_equal_the_reference_constants():
    sig = inspect.signature(U.EvalReport.__init__).parameters
    want = dict(hist_bins=100, hist_range=(-7.5, 7.5), err_range=(-3.0, 3.0), scatter_range=(-8.0, 8.0), scatter_bin_width=0.05,
                points_per_bin=1000, seed=0, device="cuda")                    # get_metrics.py:55-59, :317, :354
    assert {k: sig[k].default for k in want} == want
    assert list(sig)[:2] == ["self", "dataset_obj"]
    edges = U.EvalReport.make_scatter_edges((-8.0, 8.0), 0.05)
    assert edges.dtype == np.float64 and np.array_equal(edges, np.arange(-8.0, 8.0 + 0.05, 0.05))
    assert len(edges) == 321
    x = np.linspace(-9, 9, 10001)
    idx = np.digitize(x, edges)
    assert idx.min() == 0 and idx.max() == 321 and len(np.bincount(idx, minlength=322)) == 322
    # what the kernel is told: edges[i] == lo + i * w exactly, with w the array's own first difference
    lo, w = float(edges[0]), float(edges[1] - edges[0])
    assert np.array_equal(edges, lo + np.arange(321) * w)
    rep = U.EvalReport(_FakeDataset())
    assert rep.hist_bins == 100 and rep.hist_range == (-7.5, 7.5) and rep.err_range == (-3.0, 3.0) and rep.points_per_bin == 1000
    assert np.array_equal(rep.scatter_edges, edges) and rep.transform == 1
    sig = inspect.signature(U.evaluate_report).parameters
    assert list(sig)[:5] == ["model", "loader", "device", "dataset_obj", "use_mask"] and sig["use_mask"].default is True


# ---------------------------------------------------------------------------------------------
# EvalReport.reduce
# ---------------------------------------------------------------------------------------------
def _tables_numpy(gt, pred, valid, chunks):
    """Rows as uclstm_eval_stats defines them, from f64 arrays [B,T,C,H,W], the plane cut into `chunks` equal pieces."""
    B, T = gt.shape[:2]
    g, p, v = (a.reshape(B, T, chunks, -1) for a in (gt, pred, valid))
    d = p - g
    tab = np.zeros((B, T, chunks, ROW))
    for k, a in enumerate((np.ones_like(d), np.abs(d), d * d, d, g, g * g, p, p * p)):
        tab[..., k] = np.where(v, a, 0.0).sum(axis=-1)
    for k, a in enumerate((g, p, d)):
        tab[..., 8 + 2 * k] = np.where(v, a, np.inf).min(axis=-1)
        tab[..., 9 + 2 * k] = np.where(v, a, -np.inf).max(axis=-1)
    return tab


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1e-300)), (a, b)


@pytest.mark.parametrize("use_mask", [False, True])
def test_reduce_matches_the_get_metrics_formulas(use_mask):
    rng = np.random.default_rng(11)
    N, T, H, W = 5, 4, 16, 16
    gt = rng.normal(0.4, 2.5, (N, T, 1, H, W))
    pred = gt + rng.normal(0.1, 0.6, gt.shape) * (1.0 + np.arange(T))[None, :, None, None, None] / T      # error grows with t
    valid = rng.random(gt.shape) > 0.35 if use_mask else np.ones(gt.shape, dtype=bool)
    if use_mask:
        valid[1, 2] = False                                          # a frame without one valid pixel
    K, bins = 7, 100
    edges = U.EvalReport.make_scatter_edges((-8.0, 8.0), 0.05)
    G, Pd, D = gt[valid], pred[valid], (pred - gt)[valid]            # get_metrics.py:147-148 / :159-160, :185
    hist = np.stack([np.histogram(G, bins, (-7.5, 7.5))[0], np.histogram(Pd, bins, (-7.5, 7.5))[0], np.histogram(D, bins, (-3.0, 3.0))[0]])
    dig = np.bincount(np.digitize(G, edges), minlength=len(edges) + 1)
    scatter = np.zeros((len(edges) + 1, K, 2), dtype=np.float32)
    scatter[..., 0] = np.arange(len(edges) + 1)[:, None]
    # two add() calls: sequences 0..2 and 3..4, the plane in two chunks
    tabs = [_tables_numpy(gt[:3], pred[:3], valid[:3], 2), _tables_numpy(gt[3:], pred[3:], valid[3:], 2)]
    r = U.EvalReport.reduce(tabs, hist.astype(np.uint64), dig.astype(np.uint64), scatter, hist_range=(-7.5, 7.5),
                            err_range=(-3.0, 3.0), scatter_edges=edges, points_per_bin=K)
    assert r["n"] == float(valid.sum())
    _close(r["mae"], np.mean(np.abs(D)))                             # get_metrics.py:188-191
    _close(r["rmse"], np.sqrt(np.mean(D ** 2)))
    _close(r["mean_err"], np.mean(D))
    _close(r["std_err"], np.std(D))                                  # ddof = 0
    assert abs(r["std_err"] - np.std(D, ddof=1)) > 1e-9 * r["std_err"]
    _close([r["gt_mean"], r["gt_std"], r["gt_min"], r["gt_max"]], [G.mean(), G.std(), G.min(), G.max()])          # :320, :248
    _close([r["pred_mean"], r["pred_std"], r["pred_min"], r["pred_max"]], [Pd.mean(), Pd.std(), Pd.min(), Pd.max()])
    _close([r["err_min"], r["err_max"]], [D.min(), D.max()])         # :254-255
    # MAE per time step: the time index is axis 1 of [N,T,...] (:151 / :169, :281-297)
    t_idx = np.broadcast_to(np.arange(T)[None, :, None, None, None], gt.shape)[valid]
    for t in range(T):
        Dt = D[t_idx == t]
        assert r["per_timestep"]["n"][t] == Dt.size
        _close(r["per_timestep"]["mae"][t], np.mean(np.abs(Dt)))
        _close(r["per_timestep"]["rmse"][t], np.sqrt(np.mean(Dt ** 2)))
        _close(r["per_timestep"]["mean_err"][t], np.mean(Dt))
    # per frame (test.py:333-351), in the order added
    ps = r["per_sequence"]
    assert ps.shape == (N, T, 4) and EvalReport.SUMS == ("n", "sum_abs", "sum_sq", "sum")
    for i in range(N):
        for t in range(T):
            vd = (pred - gt)[i, t][valid[i, t]]
            assert ps[i, t, 0] == vd.size
            if vd.size:
                _close(ps[i, t, 1] / ps[i, t, 0], np.mean(np.abs(vd)))
                _close(math.sqrt(ps[i, t, 2] / ps[i, t, 0]), np.sqrt(np.mean(vd ** 2)))
                _close(ps[i, t, 3] / ps[i, t, 0], np.mean(vd))
            else:
                assert not ps[i, t].any()
    for k, h in zip(("hist_gt", "hist_pred", "hist_err"), hist):
        assert r[k].dtype == np.int64 and np.array_equal(r[k], h)
    assert np.array_equal(r["hist_edges"], np.histogram(G, bins, (-7.5, 7.5))[1]) and np.array_equal(r["err_edges"], np.linspace(-3, 3, 101))
    assert r["gt_bin_count"].dtype == np.int64 and np.array_equal(r["gt_bin_count"], dig)
    # the sample: per bin the first min(count, K) slots
    assert len(r["scatter_gt"]) == len(r["scatter_pred"]) == len(r["scatter_bin"]) == int(np.minimum(dig, K).sum())
    assert np.array_equal(np.bincount(r["scatter_bin"], minlength=len(dig)), np.minimum(dig, K))
    assert np.array_equal(r["scatter_gt"], r["scatter_bin"].astype(np.float32))


def test_reduce_of_nothing_valid_is_all_zero():
    tab = np.zeros((1, 2, 1, ROW))
    tab[..., 8:14:2], tab[..., 9:14:2] = np.inf, -np.inf
    r = U.EvalReport.reduce([tab], np.zeros((3, 4), np.uint64), np.zeros(4, np.uint64), np.zeros((4, 2, 2), np.float32),
                            hist_range=(-1, 1), err_range=(-1, 1), scatter_edges=np.array([0.0, 0.5, 1.0]), points_per_bin=2)
    assert r["n"] == 0 and r["mae"] == r["rmse"] == r["mean_err"] == r["std_err"] == 0.0 and len(r["scatter_gt"]) == 0
    assert not r["per_timestep"]["mae"].any()
