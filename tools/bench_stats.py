#!/usr/bin/env python3
"""A/B of the two dataset constructors on a synthetic Moving-MNIST-shaped ``.npz`` (N sequences of T frames, X 2 x S x S,
Y 1 x S x S with about 60 % exact zeros, written to a temporary directory), in the percentile branch the reference's main.py
takes (``min_y = max_y = None``):

    host    NPZSequenceDataset(path, min_y=None, max_y=None)        np.max, np.abs copy, 5 percentiles, arcsinh copy
    device  DeviceNPZDataset(path, min_y=None, max_y=None)          one extremes pass over X, ONE radix select over Y

One process; wall clock around each constructor (both load the same file, so the load is timed on its own and listed); the
device arm's upload of the raw arrays -- which a DeviceSequenceLoader over the host dataset would pay as well -- is timed
separately.  The constants of the two arms must agree with ``==`` or the tool stops.

Stand-alone: every histogram pass of the select (the dataset's 6 slots) and the extremes kernel on ``--elems`` f32 of three
value distributions (random normal, 60 % exact zeros, all equal), cold caches (a 1 GiB fill before every timed launch), HIP
events, median of 7 after one warm-up round; achieved bytes/s over the algorithmic bytes (4 per element: one read).

    python tools/bench_stats.py [--out profiles/dataset_stats_ab.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd import _lib as L   # noqa: E402
from unet_convlstm_amd import engine as E   # noqa: E402
from unet_convlstm_amd import ops   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="200,1000,2000", help="comma-separated N (sequences)")
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--side", type=int, default=64)
ap.add_argument("--elems", type=int, default=1 << 26, help="elements of the stand-alone kernel timings")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None, help="also append the table to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_stats: needs a GPU (no CPU fallback: a timing taken elsewhere says nothing)")
dev = torch.device("cuda", 0)
lines = []
CONSTANTS = ("x_max", "norm_const", "y_scale", "min_vel", "max_vel", "trans_min", "trans_max")


def say(msg=""):
    print(msg, flush=True)
    lines.append(msg)


def write_npz(path, n, T, S, seed=0):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, T, 2, S, S), dtype=np.float32) * 30).astype(np.float32)
    X[X < 18] = 0.0                                                      # 60 % background
    Y = (rng.standard_normal((n, T, 1, S, S), dtype=np.float32) * 2).astype(np.float32)
    Y[X[:, :, :1] == 0] = 0.0                                            # targets only where there is a sprite: 60 % exact zeros
    np.savez(path, X=X, Y=Y)
    return float((Y == 0).mean())


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def constructors(tmp, n):
    T, S = a.frames, a.side
    path = os.path.join(tmp, f"mm_{n}.npz")
    zeros = write_npz(path, n, T, S)

    def load():
        with np.load(path, allow_pickle=False) as d:
            return d["X"].astype(np.float32), d["Y"].astype(np.float32)
    (X, Y), t_load = wall(load)
    nbytes = X.nbytes + Y.nbytes
    _, t_up = wall(lambda: (torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)))
    del X, Y
    kw = dict(min_y=None, max_y=None)
    host, t_host = wall(lambda: U.NPZSequenceDataset(path, **kw))
    devds, t_dev = wall(lambda: U.DeviceNPZDataset(path, **kw))
    for name in CONSTANTS:
        if getattr(host, name) != getattr(devds, name):
            sys.exit(f"bench_stats: {name} differs: host {getattr(host, name)!r}, device {getattr(devds, name)!r}")

    def stats_only():
        x, y = devds._device_resident[dev]
        out = E._launch_extremes(x, "bench"), E.device_percentile(y, 99, absolute=True), E.device_percentile(y, [0.00001, 99.99999])
        return out
    _, t_stats = wall(stats_only)
    say(f"N = {n}, T = {T}, X 2 x {S} x {S}, Y 1 x {S} x {S}: {host.Y.size / 1e6:.1f} M targets, {100 * zeros:.1f} % exact zeros, raw arrays {nbytes / 1e6:.0f} MB")
    say(f"  np.load + astype of both arrays (inside BOTH constructors): {t_load * 1e3:9.1f} ms")
    say(f"  upload of the raw arrays alone (pageable host memory):      {t_up * 1e3:9.1f} ms ({nbytes / t_up / 1e9:.1f} GB/s)   [inside the device arm; a DeviceSequenceLoader pays it otherwise]")
    say(f"  host   NPZSequenceDataset(...):                              {t_host * 1e3:9.1f} ms   -> minus the load {1e3 * (t_host - t_load):9.1f} ms of statistics")
    say(f"  device DeviceNPZDataset(...):                                {t_dev * 1e3:9.1f} ms   -> minus load and upload {1e3 * (t_dev - t_load - t_up):9.1f} ms")
    say(f"  device statistics alone on the resident arrays (extremes + two selects, 2 syncs): {t_stats * 1e3:.2f} ms")
    say(f"  device / host constructor = {t_dev / t_host:.3f}; constants equal (==): {', '.join(f'{k} {getattr(host, k):.6g}' for k in CONSTANTS)}")
    say()
    del host, devds
    torch.cuda.empty_cache()


def kernels():
    n = a.elems
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    normal = torch.randn(n, device=dev, generator=g) * 2
    zero60 = normal * (torch.rand(n, device=dev, generator=g) >= 0.6)
    equal = torch.full((n,), 1.5, device=dev)
    ws = torch.empty(L.lib.uclstm_select_workspace_bytes() // 8, dtype=torch.int64, device=dev)
    ext = torch.empty(L.EXTREMES_WORDS, dtype=torch.int64, device=dev)
    qs = [(99, "abs"), (0.00001, "signed"), (99.99999, "signed")]
    ranks = [r for q, _ in qs for r in E.percentile_ranks(n, q)[:2]]
    kinds = [L.SELECT_ABS if k == "abs" else L.SELECT_SIGNED for _, k in qs for _ in range(2)]
    c_ranks, c_kinds = (C.c_int64 * 6)(*ranks), (C.c_int32 * 6)(*kinds)
    st, stream = L.SelectState(), torch.cuda.current_stream()

    def timed(launch, before=lambda: None):
        ts = []
        for r in range(a.rounds + 1):
            before()
            flush.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            torch.cuda.synchronize()
            if r:
                ts.append(e0.elapsed_time(e1) * 1e3)
        return ts

    say(f"kernels alone on {n / 1e6:.1f} M f32 ({4 * n / 1e6:.0f} MB algorithmic: one read), 6 slots (the dataset's: |Y| at 99, Y at 0.00001 and 99.99999), "
        f"cold caches, median of {a.rounds}")
    say(f"  {'distribution':<18}{'kernel':<14}{'median us':>10}{'min':>9}{'max':>9}{'GB/s':>8}")
    for name, v in (("random normal", normal), ("60 % exact zeros", zero60), ("all equal", equal)):
        for p in range(3):
            def before():
                L.check(L.lib.uclstm_select_begin(C.byref(st), ops._p(ws), c_ranks, c_kinds, 6, ops._stream()), "begin")
                for k in range(p):
                    L.check(L.lib.uclstm_select_accumulate(C.byref(st), k, ops._p(v), n, ops._stream()), "accumulate")
                    L.check(L.lib.uclstm_select_narrow(C.byref(st), k, ops._stream()), "narrow")
            ts = timed(lambda: L.check(L.lib.uclstm_select_accumulate(C.byref(st), p, ops._p(v), n, ops._stream()), "accumulate"), before)
            med = statistics.median(ts)
            say(f"  {name:<18}{'hist pass ' + str(p):<14}{med:>10.1f}{min(ts):>9.1f}{max(ts):>9.1f}{4 * n / med / 1e3:>8.0f}")
        L.check(L.lib.uclstm_dataset_extremes_begin(ops._p(ext), ops._stream()), "extremes_begin")
        ts = timed(lambda: L.check(L.lib.uclstm_dataset_extremes(ops._p(v), n, ops._p(ext), ops._stream()), "extremes"))
        med = statistics.median(ts)
        say(f"  {name:<18}{'extremes':<14}{med:>10.1f}{min(ts):>9.1f}{max(ts):>9.1f}{4 * n / med / 1e3:>8.0f}")
    say()


say(f"tools/bench_stats.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, numpy {np.__version__}")
torch.zeros(1, device=dev)                                               # the HIP context, before anything is timed
U.device_extremes(torch.zeros(8, device=dev))                            # ... and the code objects of the library
with tempfile.TemporaryDirectory() as tmp:
    for n in [int(s) for s in a.sizes.split(",") if s]:
        constructors(tmp, n)
kernels()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
