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
    python tools/bench_adamw.py --ema [--rounds 9] [--out profiles/ema_ab.txt]
        # the weight EMA: the optimiser step (sum of squares + uclstm_adamw_step_dev) without / with / without the
        # uclstm_ema_update sweep behind it (A/B/A), the sweep alone beside uclstm_adamw_step_groups (bytes per second of both
        # in the same run), uclstm_swap_f32 alone, and the launch log of a training step without and with an EMA attached
    python tools/bench_adamw.py --monitor [--rounds 9] [--out profiles/monitor_ab.txt]
        # the step monitor: the optimiser step without / with / without uclstm_param_stats behind it at every = 1 (A/B/A), the
        # recording call alone with and without the update column, a call that does not record alone, and the launch log of a
        # training step without and with a monitor attached
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd.optim import build_run_table, build_stat_blocks, check_run_table, check_stat_blocks   # noqa: E402

L = U._lib
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None, help="also write the table to this file")
ap.add_argument("--step", action="store_true", help="time the driver-form training step (batch 32, T 20, 64 x 64) instead")
ap.add_argument("--ema", action="store_true", help="time the optimiser step without and with the weight-EMA sweep, and the swap, instead")
ap.add_argument("--monitor", action="store_true", help="time the optimiser step without and with the per-tensor statistics call instead")
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


def ema_ab():
    with torch.device("meta"):
        model = U.TemporalUNetDualView(1, 1, base_ch=64, lstm_layers=1, use_skip_lstm=True, use_attention=False)
    n = sum(p.numel() for p in model.parameters())
    say(f"{n} parameters (the benchmark model, BASELINE.json configs[1]); cold caches: a 1 GiB fill before every measurement")
    torch.manual_seed(0)
    p = torch.randn(n, device=dev) * 0.02
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    shadow = p.clone()
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    hyper = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 1e-4, 1.0, 0, 0], dtype=torch.float32, device=dev)
    hyper_g = torch.tensor([[1.0, 0, 0, 0, 0, 0, 0, 0], [1e-4, 0.9, 0.999, 1e-8, 1e-4, 0, 0, 0]], dtype=torch.float32, device=dev)
    runs = torch.tensor([[0, n, 0]], dtype=torch.int64, device=dev)
    ema_state = torch.tensor([0.999, 10.0, 1.0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev)
    s = C.c_void_p(st.cuda_stream)

    def step():
        sq.zero_()
        L.check(L.lib.uclstm_sumsq(ptr(g), n, ptr(sq), s), "sumsq")
        L.check(L.lib.uclstm_adamw_step_dev(ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(sq), ptr(hyper), s), "dev")

    def sweep():
        L.check(L.lib.uclstm_ema_update(ptr(shadow), ptr(p), n, None, ptr(ema_state), s), "ema_update")

    def step_ema():
        step()
        sweep()

    arms = {
        "A  step (sumsq + adamw_step_dev)": step,
        "B  step + ema_update": step_ema,
        "A' step again": step,
        "G  adamw_step_groups, 1 group": lambda: L.check(L.lib.uclstm_adamw_step_groups(ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(sq), ptr(runs), 1,
                                                                                        ptr(hyper_g), 1, None, s), "groups"),
        "E  ema_update alone": sweep,
        "S  swap_f32 alone": lambda: L.check(L.lib.uclstm_swap_f32(ptr(p), ptr(shadow), n, s), "swap_f32"),
    }
    times = {k: [] for k in arms}
    for r in range(a.rounds + 1):
        for name, fn in arms.items():
            t = timed(fn)
            if r:
                times[name].append(t)
    report(arms, times)
    med = {k: statistics.median(t) for k, t in times.items()}
    names = list(arms)
    a_med = 0.5 * (med[names[0]] + med[names[2]])
    spread = max(max(times[names[0]]) - min(times[names[0]]), max(times[names[2]]) - min(times[names[2]]), abs(med[names[0]] - med[names[2]]))
    bw_g, bw_e, bw_s = 28 * n / med[names[3]] / 1e3, 12 * n / med[names[4]] / 1e3, 16 * n / med[names[5]] / 1e3
    say(f"A/B/A: step {a_med:.1f} us (A and A' medians {med[names[0]]:.1f} / {med[names[2]]:.1f}, spread {spread:.1f}), with the EMA sweep "
        f"{med[names[1]]:.1f} us: +{med[names[1]] - a_med:.1f} us = {100 * (med[names[1]] - a_med) / a_med:.1f} % of the stand-alone step")
    say(f"sweep alone / AdamW sweep alone (G): {med[names[4]]:.1f} / {med[names[3]]:.1f} us = {med[names[4]] / med[names[3]]:.3f} "
        f"(by bytes 12 / 28 = {12 / 28:.3f})")
    say(f"bytes per second: adamw_groups_kernel 28 B/parameter {bw_g:.0f} GB/s, ema_update_kernel 12 B/parameter {bw_e:.0f} GB/s, "
        f"swap_f32_kernel 16 B/parameter {bw_s:.0f} GB/s")
    if bw_e < bw_g:
        say(f"NOTE: the EMA sweep moves its bytes at {100 * bw_e / bw_g:.0f} % of adamw_groups_kernel's rate in this run (not tuned further here)")
    say(f"fusing the sweep into the AdamW kernels would save the 4 B/parameter re-read of p: at most {4 * n / (bw_e * 1e3):.1f} us of the "
        f"{med[names[4]]:.1f} us above (not built; see DESIGN.md)")
    # the launch log of a training step: what an attached EMA adds, and that nothing else moves
    torch.manual_seed(0)
    net = U.TemporalUNetDualView(1, 1, base_ch=64, lstm_layers=1, use_skip_lstm=True, use_attention=False).to(dev).train()
    opt = U.FusedAdamW(net.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    data = U.SyntheticSequences(4, 3, 64, 64, seed=1, kind="uniform", device=dev)
    logs = []
    for attach in (False, False, True):
        if attach:
            opt.attach_ema()
        U.ops.LAUNCH_LOG = []
        try:
            U.train_step(net, opt, data.x, data.y, data.mask, True)
            torch.cuda.synchronize()
            logs.append(list(U.ops.LAUNCH_LOG))
        finally:
            U.ops.LAUNCH_LOG = None
    extra = [e for e in logs[2] if e[0] == "ema"]
    same = logs[0] == logs[1] == [e for e in logs[2] if e[0] != "ema"]
    say(f"launch log of one train_step (base_ch 64, batch 4, T 3, 64 x 64): {len(logs[0])} entries without an EMA, none of kind 'ema'; with "
        f"attach_ema() the same entries {'in the same order' if same else 'DIFFER'} plus {extra}")
    return same and extra == [("ema", "update", False)] and not [e for e in logs[0] if e[0] == "ema"]



def monitor_ab():
    with torch.device("meta"):
        model = U.TemporalUNetDualView(1, 1, base_ch=64, lstm_layers=1, use_skip_lstm=True, use_attention=False)
    sizes = [p.numel() for p in model.parameters()]
    n = sum(sizes)
    chunk = int(L.lib.uclstm_param_stats_chunk())
    blocks_h, tensors_h = build_stat_blocks(sizes, chunk)
    check_stat_blocks(blocks_h, tensors_h, n, chunk)
    say(f"{n} parameters in {len(sizes)} tensors (the benchmark model, BASELINE.json configs[1]): {blocks_h.shape[0]} blocks of up to {chunk} "
        f"elements; cold caches: a 1 GiB fill before every measurement")
    torch.manual_seed(0)
    p = torch.randn(n, device=dev) * 0.02
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    prev = p.clone()
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    hyper = torch.tensor([1e-4, 0.9, 0.999, 1e-8, 1e-4, 1.0, 0, 0], dtype=torch.float32, device=dev)
    blocks, tensors = torch.from_numpy(blocks_h).to(dev), torch.from_numpy(tensors_h).to(dev)
    history = 8
    partials = torch.zeros((blocks_h.shape[0], 8), dtype=torch.float64, device=dev)
    ring = torch.zeros((history, len(sizes), 8), dtype=torch.float64, device=dev)
    meta = torch.zeros((history, 4), dtype=torch.float64, device=dev)
    state_1 = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)
    state_0 = torch.tensor([1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)
    state_never = torch.tensor([(1 << 24) - 1, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)
    s = C.c_void_p(st.cuda_stream)

    def step():
        sq.zero_()
        L.check(L.lib.uclstm_sumsq(ptr(g), n, ptr(sq), s), "sumsq")
        L.check(L.lib.uclstm_adamw_step_dev(ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(sq), ptr(hyper), s), "dev")

    def stats(prev_t, state):
        return lambda: L.check(L.lib.uclstm_param_stats(ptr(p), ptr(g), None if prev_t is None else ptr(prev_t), n, ptr(blocks),
                                                        int(blocks_h.shape[0]), ptr(tensors), len(sizes), ptr(partials), ptr(ring), ptr(meta),
                                                        history, ptr(sq), None, ptr(state), s), "param_stats")

    record = stats(prev, state_1)

    def step_monitor():
        step()
        record()

    arms = {
        "A  step (sumsq + adamw_step_dev)": step,
        "B  step + param_stats, every 1": step_monitor,
        "A' step again": step,
        "M1 param_stats alone, updates": record,
        "M0 param_stats alone, no updates": stats(None, state_0),
        "N  param_stats, not recording": stats(prev, state_never),
    }
    times = {k: [] for k in arms}
    for r in range(a.rounds + 1):
        for name, fn in arms.items():
            t = timed(fn)
            if r:
                times[name].append(t)
    report(arms, times)
    med = {k: statistics.median(t) for k, t in times.items()}
    names = list(arms)
    a_med = 0.5 * (med[names[0]] + med[names[2]])
    spread = max(max(times[names[0]]) - min(times[names[0]]), max(times[names[2]]) - min(times[names[2]]), abs(med[names[0]] - med[names[2]]))
    say(f"A/B/A: step {a_med:.1f} us (A and A' medians {med[names[0]]:.1f} / {med[names[2]]:.1f}, spread {spread:.1f}), with the record "
        f"{med[names[1]]:.1f} us: +{med[names[1]] - a_med:.1f} us = {100 * (med[names[1]] - a_med) / a_med:.1f} % of the stand-alone step")
    say(f"bytes per second: recording sweep with updates 16 B/parameter {16 * n / med[names[3]] / 1e3:.0f} GB/s, without 8 B/parameter "
        f"{8 * n / med[names[4]] / 1e3:.0f} GB/s (both launches of the call in the time); a call that does not record: "
        f"{med[names[5]]:.1f} us for its two launches")
    torch.cuda.synchronize()
    counts = [int(x[1]) for x in (state_1.cpu(), state_0.cpu(), state_never.cpu())], [int(x[2]) for x in (state_1.cpu(), state_0.cpu(), state_never.cpu())]
    say(f"calls seen / records made by the three states: {counts[0]} / {counts[1]}")
    # the launch log of a training step: what an attached monitor adds, and that nothing else moves
    torch.manual_seed(0)
    net = U.TemporalUNetDualView(1, 1, base_ch=64, lstm_layers=1, use_skip_lstm=True, use_attention=False).to(dev).train()
    opt = U.FusedAdamW(net.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    data = U.SyntheticSequences(4, 3, 64, 64, seed=1, kind="uniform", device=dev)
    logs = []
    for attach in (False, False, True):
        if attach:
            opt.attach_monitor(names=net.named_parameters())
        U.ops.LAUNCH_LOG = []
        try:
            U.train_step(net, opt, data.x, data.y, data.mask, True)
            torch.cuda.synchronize()
            logs.append(list(U.ops.LAUNCH_LOG))
        finally:
            U.ops.LAUNCH_LOG = None
    extra = [e for e in logs[2] if e[0] == "monitor"]
    same = logs[0] == logs[1] == [e for e in logs[2] if e[0] != "monitor"]
    say(f"launch log of one train_step (base_ch 64, batch 4, T 3, 64 x 64): {len(logs[0])} entries without a monitor, none of kind 'monitor'; "
        f"with attach_monitor() the same entries {'in the same order' if same else 'DIFFER'} plus {extra}")
    say(opt.monitor.report(top=3))
    return same and extra == [("monitor", "stats", True, False)] and not [e for e in logs[0] if e[0] == "monitor"] \
        and counts[1][2] == 0 and counts[1][0] == counts[0][0]


ok = monitor_ab() if a.monitor else ema_ab() if a.ema else step_ab() if a.step else optimiser_ab()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
