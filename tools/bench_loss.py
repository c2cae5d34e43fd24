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

--weights: the per-plane-weight kernels (uclstm_loss_spec_fwd_pw / _fwd_ordered_pw / _bwd_pw, loss.WeightedLossSpec) against the
plain LossSpec kernels at the reference's parameters, A B A per round, on [32,20,1,64,64] (mask per plane) and [32,20,3,64,64]
(mask [32,20,1,64,64], the _bc kernels as the plain side).  Every launch of a window takes the next of enough copies of its
buffers to exceed 512 MB, so no launch finds its planes in the last-level cache.

    python tools/bench_loss.py --weights [--rounds 7] [--reps 200] [--out profiles/loss_plane_weights_ab.txt]
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
ap.add_argument("--weights", action="store_true", help="A/B/A of the per-plane-weight kernels against the plain LossSpec kernels")
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


W_GROUPS = ["A plain", "B weighted", "A' plain again"]
W_SHAPES = [(32, 20, 1, 64, 64), (32, 20, 3, 64, 64)]
W_KERNELS = ("fwd", "fwd_ordered", "bwd")


def bench_weights(shape):
    B, T, Cy, H, W = shape
    planes, n = B * T * Cy, B * T * Cy * H * W
    nbytes = {"fwd": 4 * (2 * n + n // Cy), "fwd_ordered": 4 * (2 * n + n // Cy), "bwd": 4 * (3 * n + n // Cy)}
    copies = max(2, -(-(512 << 20) // nbytes["fwd"]))
    torch.manual_seed(0)
    sets = [(torch.randn(shape, device=dev), torch.randn(shape, device=dev), (torch.rand((B, T, 1, H, W), device=dev) > 0.3).float(),
             torch.empty(shape, device=dev)) for _ in range(copies)]
    spec = U.WeightedLossSpec(frame_weights=tuple(0.0 if t < 2 else 0.5 + 0.05 * t for t in range(T)),
                              channel_weights=None if Cy == 1 else (0.3, 0.3, 2.0))
    q = ops.plane_weight_table(spec, sets[0][0])[0]
    desc = ops.loss_spec_desc(spec)
    rows = int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W))
    sums, partials = torch.zeros(4, dtype=torch.float64, device=dev), torch.empty((rows, 4), dtype=torch.float64, device=dev)
    coefs = torch.tensor([1.0 / n, 0.005 / n], device=dev)
    turn = [0]

    def arm(group, kernel):
        weighted, bc = group.startswith("B"), Cy > 1
        lib, d = L.lib, C.byref(desc)

        def fn():
            yp, y, m, grad = sets[turn[0] % copies]
            turn[0] += 1
            if weighted:
                if kernel == "fwd":
                    rc = lib.uclstm_loss_spec_fwd_pw(d, ptr(yp), ptr(y), ptr(m), ptr(q), q.numel(), ptr(sums), planes, H, W, Cy, s)
                elif kernel == "fwd_ordered":
                    rc = lib.uclstm_loss_spec_fwd_ordered_pw(d, ptr(yp), ptr(y), ptr(m), ptr(q), q.numel(), ptr(partials), ptr(sums), 0, planes, H, W, Cy, s)
                else:
                    rc = lib.uclstm_loss_spec_bwd_pw(d, ptr(yp), ptr(y), ptr(m), ptr(q), q.numel(), ptr(coefs), ptr(grad), planes, H, W, Cy, s)
            elif bc:
                if kernel == "fwd":
                    rc = lib.uclstm_loss_spec_fwd_bc(d, ptr(yp), ptr(y), ptr(m), ptr(sums), planes, H, W, Cy, s)
                elif kernel == "fwd_ordered":
                    rc = lib.uclstm_loss_spec_fwd_ordered_bc(d, ptr(yp), ptr(y), ptr(m), ptr(partials), ptr(sums), 0, planes, H, W, Cy, s)
                else:
                    rc = lib.uclstm_loss_spec_bwd_bc(d, ptr(yp), ptr(y), ptr(m), ptr(coefs), ptr(grad), planes, H, W, Cy, s)
            else:
                if kernel == "fwd":
                    rc = lib.uclstm_loss_spec_fwd(d, ptr(yp), ptr(y), ptr(m), ptr(sums), planes, H, W, s)
                elif kernel == "fwd_ordered":
                    rc = lib.uclstm_loss_spec_fwd_ordered(d, ptr(yp), ptr(y), ptr(m), ptr(partials), ptr(sums), 0, planes, H, W, s)
                else:
                    rc = lib.uclstm_loss_spec_bwd(d, ptr(yp), ptr(y), ptr(m), ptr(coefs), ptr(grad), planes, H, W, s)
            L.check(rc, f"{group} {kernel}")
        return fn

    arms = {(g, k): arm(g, k) for g in W_GROUPS for k in W_KERNELS}
    times = {key: [] for key in arms}
    for r in range(a.rounds + 1):
        for g in W_GROUPS:
            for k in W_KERNELS:
                t, _ = window(arms[(g, k)])
                if r:                                       # round 0 warms up
                    times[(g, k)].append(t)
    say(f"\n{list(shape)}, mask [{B}, {T}, 1, {H}, {W}]{' (broadcast, mask_div 3)' if Cy > 1 else ''}: {n} elements, {copies} copies of the "
        f"buffers in rotation; {nbytes['fwd'] / 1e6:.1f} MB per forward launch, {nbytes['bwd'] / 1e6:.1f} MB per backward launch, "
        f"table {q.numel() * 4} bytes")
    say(f"{'group':18s} {'kernel':12s} {'median':>8s} {'min':>8s} {'max':>8s} {'GB/s':>8s}   [us per launch; {a.rounds} rounds of {a.reps} launches]")
    med = {}
    for k in W_KERNELS:
        for g in W_GROUPS:
            t = times[(g, k)]
            med[(g, k)] = statistics.median(t)
            say(f"{g:18s} {k:12s} {med[(g, k)]:8.2f} {min(t):8.2f} {max(t):8.2f} {nbytes[k] / med[(g, k)] / 1e3:8.0f}")
    for k in W_KERNELS:
        a0, a1, b = med[(W_GROUPS[0], k)], med[(W_GROUPS[2], k)], med[(W_GROUPS[1], k)]
        spread, d = abs(a0 - a1), b - max(a0, a1)
        say(f"  {k:12s} B median - slower A median = {d:+6.2f} us ({100 * d / max(a0, a1):+.1f} %), A / A' spread {spread:.2f} us: "
            f"{'within the spread or faster' if d <= spread else 'SLOWER than plain by more than the spread'}")


if a.weights:
    say(f"per-plane-weight loss kernels against the plain LossSpec kernels on {torch.cuda.get_device_name(0)}, reference parameters, "
        f"groups in A B A order per round, buffers rotated past the last-level cache")
    for shape in W_SHAPES:
        bench_weights(shape)
else:
    say(f"loss kernels stand-alone on {torch.cuda.get_device_name(0)}, warm, groups in A B C D A order per round")
    for shape in SHAPES:
        for masked in (True, False):
            bench(shape, masked)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
