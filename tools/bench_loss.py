#!/usr/bin/env python3
"""The loss kernels stand-alone: the reference's (uclstm_loss_fwd / uclstm_loss_bwd) and the LossSpec ones (uclstm_loss_spec_fwd /
uclstm_loss_spec_bwd) at the reference's parameters, at LossSpec.masked_mse() and at Huber, on the planes of the benchmark
([32*20, 64, 64]) and of a 256 x 256 run ([4*12, 256, 256]), masked and unmasked.  One process, warm, HIP events around a window
of --reps launches of one kernel; the groups run in the order A B C D A inside every round, so the table holds the legacy group
twice and the difference of its two medians is the spread a difference between groups has to exceed.

    A   legacy kernels                         C   spec kernels, masked_mse (L2, w = 1, no gradient term)
    B   spec kernels, reference parameters     D   spec kernels, Huber delta 1, power 2, gradient term

Bytes per launch are the algorithm's: each input plane once (y_pred, y, the mask when there is one) and, backward, the gradient
plane; the neighbour reads of the gradient term hit lines the sweep loads anyway.

    python tools/bench_loss.py [--rounds 7] [--reps 200] [--out profiles/loss_spec_ab.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd import ops   # noqa: E402

L = U._lib
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=200, help="launches per timed window")
ap.add_argument("--out", default=None, help="also append the table to this file")
a = ap.parse_args()
dev = torch.device("cuda:0")
st = torch.cuda.current_stream()
s = C.c_void_p(st.cuda_stream)
lines = []

SPECS = {
    "B spec @ reference": U.LossSpec(),
    "C spec @ masked_mse": U.LossSpec.masked_mse(),
    "D spec @ huber p2": U.LossSpec(point="huber", delta=1.0, weight_power=2),
}
GROUPS = ["A legacy", *SPECS, "A' legacy again"]
SHAPES = [(32 * 20, 64, 64), (4 * 12, 256, 256)]


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def window(fn):
    """Mean time of one launch in a window of a.reps back-to-back launches [us]: (between device events, on the host to enqueue).
    Where the two agree the window measures the host's launch rate, not the kernel."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    h0 = time.perf_counter()
    for _ in range(a.reps):
        fn()
    h1 = time.perf_counter()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.reps, (h1 - h0) * 1e6 / a.reps


def launches(group, yp, y, m, sums, coefs, grad, planes, H, W):
    if group.startswith("A"):
        fwd = lambda: L.check(L.lib.uclstm_loss_fwd(ptr(yp), ptr(y), ptr(m), ptr(sums), planes, H, W, s), "loss_fwd")   # noqa: E731
        bwd = lambda: L.check(L.lib.uclstm_loss_bwd(ptr(yp), ptr(y), ptr(m), ptr(coefs), ptr(grad), planes, H, W, s), "loss_bwd")   # noqa: E731
        return fwd, bwd
    desc = ops.loss_spec_desc(SPECS[group])
    fwd = lambda: L.check(L.lib.uclstm_loss_spec_fwd(C.byref(desc), ptr(yp), ptr(y), ptr(m), ptr(sums), planes, H, W, s), "loss_spec_fwd")   # noqa: E731
    bwd = lambda: L.check(L.lib.uclstm_loss_spec_bwd(C.byref(desc), ptr(yp), ptr(y), ptr(m), ptr(coefs), ptr(grad), planes, H, W, s),   # noqa: E731
                          "loss_spec_bwd")
    return fwd, bwd


def bench(shape, masked):
    planes, H, W = shape
    n = planes * H * W
    torch.manual_seed(0)
    yp, y = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    m = (torch.rand(shape, device=dev) > 0.3).float() if masked else None
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    coefs = torch.tensor([1.0 / n, 0.005 / n], device=dev)
    grad = torch.empty(shape, device=dev)
    arms = {g: launches(g, yp, y, m, sums, coefs, grad, planes, H, W) for g in GROUPS}
    times = {(g, k): [] for g in GROUPS for k in ("fwd", "bwd")}
    host = {(g, k): [] for g in GROUPS for k in ("fwd", "bwd")}
    for r in range(a.rounds + 1):
        for g in GROUPS:
            for k, fn in zip(("fwd", "bwd"), arms[g]):
                t, h = window(fn)
                if r:                                   # round 0 warms up (code-object load, first-launch attributes)
                    times[(g, k)].append(t)
                    host[(g, k)].append(h)
    nbytes = {"fwd": 4 * n * (3 if masked else 2), "bwd": 4 * n * (4 if masked else 3)}
    say(f"\n[{planes}, {H}, {W}] {'masked' if masked else 'unmasked'}: {n} elements; {nbytes['fwd'] / 1e6:.1f} MB per forward launch, "
        f"{nbytes['bwd'] / 1e6:.1f} MB per backward launch")
    say(f"{'group':22s} {'kernel':4s} {'median':>8s} {'min':>8s} {'max':>8s} {'GB/s':>8s} {'enqueue':>8s}   [us per launch; {a.rounds} rounds of {a.reps} launches]")
    med = {}
    for k in ("fwd", "bwd"):
        for g in GROUPS:
            t = times[(g, k)]
            med[(g, k)] = statistics.median(t)
            say(f"{g:22s} {k:4s} {med[(g, k)]:8.2f} {min(t):8.2f} {max(t):8.2f} {nbytes[k] / med[(g, k)] / 1e3:8.0f} {statistics.median(host[(g, k)]):8.2f}")
    for k in ("fwd", "bwd"):
        a0, a1 = med[(GROUPS[0], k)], med[(GROUPS[-1], k)]
        spread, base = abs(a0 - a1), min(a0, a1)
        worst = max(a0, a1)
        for g in SPECS:
            d = med[(g, k)] - worst
            say(f"  {k} {g:22s} median - slower legacy median = {d:+6.2f} us (legacy A / A' spread {spread:.2f} us, faster legacy {base:.2f} us): "
                f"{'within the spread or faster' if d <= spread else 'SLOWER than legacy by more than the spread'}")


say(f"loss kernels stand-alone on {torch.cuda.get_device_name(0)}, warm, groups in A B C D A order per round")
for shape in SHAPES:
    for masked in (True, False):
        bench(shape, masked)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
