#!/usr/bin/env python3
"""Pack / unpack kernel throughput on the benchmark model's panels (GB/s of f32 read + bf16 written).

    python tools/bench_pack.py                    the pack kernels on the model's panels
    python tools/bench_pack.py --unpack-first     the first-layer weight-gradient unpack (4096 elements x 1000 slabs, accumulate):
                                                  atomic slab groups against the ordered two-launch form, arms alternating
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd import ops   # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def unpack_first(rounds=9, nslab=1000):
    import ctypes as C
    from unet_convlstm_amd import _lib as L
    d = ops.im2col_pack_desc(64, 1, 16)
    total = d.N * d.Ktot
    slabs = torch.randn(nslab, d.N, d.Ktot, device="cuda")
    grad = torch.zeros(64, 1, 3, 3, device="cuda")
    groups = int(L.lib.uclstm_unpack_wgrad_ordered_groups(C.byref(d), nslab))
    scratch = torch.empty(groups, total, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arms = {"atomic  uclstm_unpack_wgrad": lambda: L.check(L.lib.uclstm_unpack_wgrad(C.byref(d), ops._p(slabs), nslab, total, ops._p(grad), 1, st), "unpack"),
            "ordered uclstm_unpack_wgrad_ordered": lambda: L.check(L.lib.uclstm_unpack_wgrad_ordered(C.byref(d), ops._p(slabs), nslab, total, ops._p(scratch),
                                                                                                 ops._p(grad), 1, st), "unpack_ordered")}
    times = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    for _ in range(rounds):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / 20)
    print(f"first-layer unpack, {total} elements x {nslab} slabs, accumulate, {groups} slab groups; us per call (20 back to back), {rounds} alternating rounds")
    for k, v in times.items():
        v = sorted(v)
        print(f"{k:40s} median {v[len(v) // 2]:8.2f}  min {v[0]:8.2f}  max {v[-1]:8.2f}")


if "--unpack-first" in sys.argv:
    unpack_first()
    sys.exit(0)

cases = []
for name, Hd in (("temporal", 1024), ("skip3", 512), ("skip2", 256)):
    w = torch.randn(4 * Hd, 2 * Hd, 3, 3, device="cuda")
    cases += [(f"{name} lstm fwd", ops.lstm_pack_desc(Hd, Hd), w, 0), (f"{name} lstm dgrad h", ops.lstm_dgrad_pack_desc(Hd, Hd, Hd), w, Hd * 9),
              (f"{name} lstm dgrad x", ops.lstm_dgrad_pack_desc(Hd, Hd, Hd), w, 0)]
for co, ci in ((1024, 1024), (512, 1024), (512, 512), (256, 256), (128, 128), (64, 64)):
    w = torch.randn(co, ci, 3, 3, device="cuda")
    cases += [(f"conv {ci}->{co} fwd", ops.conv_pack_desc(co, ci, [ci], [ci]), w, 0), (f"conv {ci}->{co} dgrad", ops.conv_dgrad_pack_desc(co, ci, ci), w, 0)]
tot_t = tot_b = 0.0
for name, d, w, off in cases:
    t = timeit(lambda: ops.pack_weights(d, w, off))
    nbytes = d.N * d.Ktot * 2 + d.N * d.Ktot * 4 * 1.0
    tot_t += t
    tot_b += nbytes
    print(f"{name:28s} panel {d.N:5d} x {d.Ktot:6d}  {t * 1e6:8.1f} us  {nbytes / t / 1e9:8.1f} GB/s")
print(f"sum {tot_t * 1e3:.3f} ms, {tot_b / tot_t / 1e9:.1f} GB/s")
