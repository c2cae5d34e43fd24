#!/usr/bin/env python3
"""The optimiser entry points stand-alone, on buffers of the benchmark model's size (the tensor sizes of
TemporalUNetDualView(1, 1, 64, use_skip_lstm=True): 130 140 545 f32), cold caches (a 1 GiB fill before every launch, as
tools/bench_boundary.py does), HIP events, the arms alternating inside every round of ONE process:

    A   uclstm_adamw_step_dev                      (the single-group capturable step)
    B1  uclstm_adamw_step_groups, one group, one run
    B2  uclstm_adamw_step_groups, two groups "weights / BatchNorm + bias" in registration order (the interleaved runs)
    B3  B2 with scale_state (loss scaling)

Prints medians and min - max per arm and whether each B median exceeds A's median by more than A's own min - max spread.

    python tools/bench_adamw.py [--rounds 9] [--out profiles/adamw_groups_ab.txt]
    python tools/bench_adamw.py --step [--rounds 5]     # driver-form train_step, ConvLSTM weights frozen vs all trainable
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd.optim import build_run_table, check_run_table   # noqa: E402

L = U._lib
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None, help="also write the table to this file")
ap.add_argument("--step", action="store_true", help="time the driver-form training step (batch 32, T 20, 64 x 64) instead")
a = ap.parse_args()
dev = torch.device("cuda:0")
st = torch.cuda.current_stream()
flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
lines = []


def say(msg):
    print(msg, flush=True)
    lines.append(msg)


def timed(fn):
    flush.fill_(1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def report(arms, times, unit="us"):
    say(f"{'arm':34s} {'median':>10s} {'min':>10s} {'max':>10s}   [{unit}], {a.rounds} alternating rounds")
    for name in arms:
        t = times[name]
        say(f"{name:34s} {statistics.median(t):10.1f} {min(t):10.1f} {max(t):10.1f}")


def ptr(t):
    return C.c_void_p(t.data_ptr())


def optimiser_ab():
    with torch.device("meta"):
        model = U.TemporalUNetDualView(1, 1, base_ch=64, lstm_layers=1, use_skip_lstm=True, use_attention=False)
    sizes = [p.numel() for p in model.parameters()]
    group = [0 if p.ndim > 1 else 1 for p in model.parameters()]
    n = sum(sizes)
    table = build_run_table(sizes, group)
    check_run_table(table, n, 2)
    say(f"{n} parameters in {len(sizes)} tensors; two groups (weights / BatchNorm + bias): {len(table)} runs, shortest "
        f"{min(e - b for b, e, _ in table)} elements")
    torch.manual_seed(0)
    p = torch.randn(n, device=dev) * 0.02
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    L.check(L.lib.uclstm_sumsq(ptr(g), n, ptr(sq), None), "sumsq")
    grp = [1e-4, 0.9, 0.999, 1e-8, 1e-4, 0, 0, 0]
    hyper_a = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 1e-4, 1.0, 0, 0], dtype=torch.float32, device=dev)
    hyper_1 = torch.tensor([[1.0, 0, 0, 0, 0, 0, 0, 0], grp], dtype=torch.float32, device=dev)
    hyper_2 = torch.tensor([[1.0, 0, 0, 0, 0, 0, 0, 0], grp, grp[:4] + [0.0, 0, 0, 0]], dtype=torch.float32, device=dev)
    hyper_3 = hyper_2.clone()
    runs_1 = torch.tensor([[0, n, 0]], dtype=torch.int64, device=dev)
    runs_2 = torch.tensor(table, dtype=torch.int64, device=dev)
    state = torch.tensor([1.0, 0.0, 0.0], device=dev)          # scale 1: g is read as it is, like the other arms
    s = C.c_void_p(st.cuda_stream)

    def groups(runs, hyper, n_groups, scale):
        return lambda: L.check(L.lib.uclstm_adamw_step_groups(ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(sq), ptr(runs), int(runs.shape[0]),
                                                              ptr(hyper), n_groups, None if scale is None else ptr(scale), s), "groups")
    arms = {
        "A  adamw_step_dev": lambda: L.check(L.lib.uclstm_adamw_step_dev(ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(sq), ptr(hyper_a), s), "dev"),
        "B1 groups, 1 group / 1 run": groups(runs_1, hyper_1, 1, None),
        f"B2 groups, 2 groups / {len(table)} runs": groups(runs_2, hyper_2, 2, None),
        "B3 = B2 + scale_state": groups(runs_2, hyper_3, 2, state),
    }
    times = {k: [] for k in arms}
    for r in range(a.rounds + 1):
        for name, fn in arms.items():
            t = timed(fn)
            if r:                                   # round 0 warms up (code-object load, first-launch attributes)
                times[name].append(t)
    report(arms, times)
    names = list(arms)
    ta = times[names[0]]
    med_a, spread = statistics.median(ta), max(ta) - min(ta)
    say(f"28 B / parameter: A moves {28 * n / med_a / 1e3:.0f} GB/s; A's own min - max spread {spread:.1f} us")
    ok = True
    for name in names[1:]:
        d = statistics.median(times[name]) - med_a
        good = d <= spread
        ok = ok and good
        say(f"{name:34s} median - A median = {d:+7.1f} us  ({'within' if good else 'BEYOND'} A's spread)")
    return ok


def step_ab():
    lstm = ("temporal.layers.0.conv.weight", "lstm_skip3.layers.0.conv.weight", "lstm_skip2.layers.0.conv.weight")
    data = U.SyntheticSequences(32, 20, 64, 64, seed=1, kind="uniform", device=dev)
    cases = {}
    for name, frozen in (("all trainable", ()), ("ConvLSTM weights frozen", lstm)):
        torch.manual_seed(0)
        model = U.TemporalUNetDualView(1, 1, base_ch=64, lstm_layers=1, use_skip_lstm=True, use_attention=False).to(dev).train()
        named = dict(model.named_parameters())
        for k in frozen:
            named[k].requires_grad_(False)
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
        cases[name] = (model, opt)
    times = {k: [] for k in cases}
    for r in range(a.rounds + 2):
        for name, (model, opt) in cases.items():
            t = timed(lambda: [U.train_step(model, opt, data.x, data.y, data.mask, True) for _ in range(5)]) / 5e3
            if r >= 2:
                times[name].append(t)
    say("driver-form training step (batch 32, T 20, 64 x 64, base_ch 64, bf16), mean of 5 consecutive steps per measurement")
    report(cases, times, unit="ms")
    return True


ok = step_ab() if a.step else optimiser_ab()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
