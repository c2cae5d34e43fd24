"""Shared by tests/test_vector_report_host.py and tests/test_gpu_vector_report.py: a VectorNPZDataset without a file, and the f64
statement of the vector quantities of uclstm_eval_stats_vec (include/uclstm.h) on de-normalised components."""
import numpy as np

import unet_convlstm_amd as U

_FWD = {"asinh": lambda v, s: np.arcsinh(v / s), "signed_log": lambda v, s: np.sign(v) * np.log1p(np.abs(v) / s), None: lambda v, s: v}


def vector_dataset(axes, y_transform="asinh", y_scale=(2.0, 2.5, 1.0, 3.0), min_y=(-9.5, -9.75, -4.0, -10.0), max_y=(9.5, 10.0, 4.5, 10.25)):
    """The attributes of a VectorNPZDataset that the report, de-normalisation and normalise64 read; trans_min / trans_max as its
    constructor derives them from explicit bounds.  Every channel has constants of its own."""
    ds = object.__new__(U.VectorNPZDataset)
    Cy = len(axes)
    ds.Cy, ds.axes, ds.y_transform = Cy, tuple(axes), y_transform
    w = [c for c, a in enumerate(axes) if a is not None and a[1] == "w"]
    h = [c for c, a in enumerate(axes) if a is not None and a[1] == "h"]
    ds.w_channel, ds.h_channel = (w[0] if w else None), (h[0] if h else None)
    ds.y_scale = np.asarray(y_scale[:Cy], dtype=np.float64)
    ds.min_vel, ds.max_vel = np.asarray(min_y[:Cy], dtype=np.float64), np.asarray(max_y[:Cy], dtype=np.float64)
    ds.trans_min = np.array([float(_FWD[y_transform](np.float64(v), s)) for v, s in zip(ds.min_vel, ds.y_scale)])
    ds.trans_max = np.array([float(_FWD[y_transform](np.float64(v), s)) for v, s in zip(ds.max_vel, ds.y_scale)])
    return ds


def sign(axis):
    return -1.0 if axis[0] == "-" else 1.0


def vector_quantities(ds, gt, pr):
    """``gt``, ``pr``: de-normalised ``[..., Cy, H, W]`` (any float dtype) -> f64 ``(s_g, s_p, ds, epe, dtheta_deg)`` over ``[..., H, W]``
    in the image frame: a = s_w * v[w] along +column, b = s_h * v[h] along +row."""
    w, h = ds.w_channel, ds.h_channel
    gt, pr = np.asarray(gt, dtype=np.float64), np.asarray(pr, dtype=np.float64)
    ga, gb = sign(ds.axes[w]) * gt[..., w, :, :], sign(ds.axes[h]) * gt[..., h, :, :]
    pa, pb = sign(ds.axes[w]) * pr[..., w, :, :], sign(ds.axes[h]) * pr[..., h, :, :]
    sg, sp = np.hypot(ga, gb), np.hypot(pa, pb)
    th = np.degrees(np.arctan2(ga * pb - gb * pa, ga * pa + gb * pb))
    return sg, sp, sp - sg, np.hypot(pa - ga, pb - gb), th
