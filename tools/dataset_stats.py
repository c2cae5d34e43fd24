#!/usr/bin/env python3
"""The dataset's normalisation constants and what the reference's get_data_min_max.py prints (min / max / non-zero count of the
arrays), computed on the device: ``DeviceNPZDataset`` for the constants (one extremes pass over X, one radix select over Y),
``device_extremes`` for the rest.  The 100-bin histogram plot of get_data_min_max.py is not produced.

    python tools/dataset_stats.py --npz FILE [--min-y V --max-y V] [--transform asinh|signed_log|none]
                                  [--lower 0.00001 --upper 99.99999] [--scale V | --scale-percentile 99] [--max-resident-bytes N]

Without --min-y / --max-y the percentile branch runs, as the reference's main.py builds its dataset.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd import engine as E   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--npz", required=True)
ap.add_argument("--min-y", type=float, default=None)
ap.add_argument("--max-y", type=float, default=None)
ap.add_argument("--transform", default="asinh", choices=["asinh", "signed_log", "none"])
ap.add_argument("--lower", type=float, default=0.00001)
ap.add_argument("--upper", type=float, default=99.99999)
ap.add_argument("--scale", type=float, default=None, help="y_transform_scale (default: the --scale-percentile of |Y|)")
ap.add_argument("--scale-percentile", type=float, default=99)
ap.add_argument("--max-resident-bytes", type=int, default=None, help="stream the arrays in chunks when they are larger than this")
ap.add_argument("--chunk-bytes", type=int, default=256 << 20)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dataset_stats: needs a GPU (this package has no CPU path; NPZSequenceDataset computes the same constants on the host)")

ds = U.DeviceNPZDataset(a.npz, lower_percentile=a.lower, upper_percentile=a.upper, min_y=a.min_y, max_y=a.max_y,
                        y_transform=None if a.transform == "none" else a.transform, y_transform_scale=a.scale,
                        y_transform_percentile=a.scale_percentile, max_resident_bytes=a.max_resident_bytes, chunk_bytes=a.chunk_bytes)
print(f"{a.npz}: N = {ds.N}, T = {ds.T}, X {tuple(ds.X.shape[2:])}, Y {tuple(ds.Y.shape[2:])}")
for name in ("x_max", "norm_const", "y_scale", "min_vel", "max_vel", "trans_min", "trans_max"):
    print(f"  {name:<11}{getattr(ds, name)!r}")
resident = next(iter(getattr(ds, "_device_resident", {}).values()), None)
chunk = max(a.chunk_bytes // 4, 1)
for label, arr, t in (("X", ds.X, resident and resident[0]), ("Y", ds.Y, resident and resident[1])):
    s = U.device_extremes(t if t is not None else E._HostChunks(arr, chunk, "cuda"))
    print(f"  {label}: min {s['min']!r}, max {s['max']!r}, non-zero {s['nonzero']} of {s['count']}, NaN {s['nan_count']}")
