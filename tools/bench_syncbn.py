#!/usr/bin/env python3
"""A/B of the eager training step with SyncBatchNorm off and on, at world size 1 over RCCL, on the benchmark workload
(BASELINE.json configs[1]: TemporalUNetDualView(base_ch=64, use_skip_lstm=True), 32 sequences of 20 frames 2 x 64 x 64, bf16).

With one rank the all-reduce moves nothing: this measures what the switch ADDS to a step on every rank -- four small launches
and two collective calls per BatchNorm stage, and the host time to issue them -- and NOT the exchange between GPUs, which needs
a multi-GPU machine.

Both arms run ``train_step`` over the SAME model, FusedAdamW and FlatDDP wrapper inside one process and alternate round by round
(clock, allocator and cache state are shared); a round is ``--steps`` steps timed with a host clock around them and a device
synchronisation at both ends.  Two warm-up rounds per arm, then ``--rounds`` timed ones per arm.

    python tools/bench_syncbn.py [--rounds 5] [--steps 10] [--out profiles/syncbn_ab.txt]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd import ops   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5, help="timed rounds per arm (>= 3)")
ap.add_argument("--steps", type=int, default=10, help="training steps per round")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--seq", type=int, default=20)
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--base-ch", type=int, default=64)
ap.add_argument("--port", type=int, default=29711)
ap.add_argument("--out", default=None, help="also append the table to this file")
a = ap.parse_args()
if a.rounds < 3:
    ap.error("--rounds must be at least 3")
if not torch.cuda.is_available():
    sys.exit("bench_syncbn: needs a GPU (no CPU fallback: a timing taken elsewhere says nothing)")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
lines = []


def say(msg=""):
    print(msg, flush=True)
    lines.append(msg)


dist.init_process_group("nccl", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{a.port}", device_id=dev,
                        timeout=datetime.timedelta(seconds=120))
try:
    say(f"tools/bench_syncbn.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, RCCL world size 1")
    say(f"workload: TemporalUNetDualView(base_ch={a.base_ch}, use_skip_lstm=True), batch {a.batch}, T = {a.seq}, 2 x {a.size} x {a.size}, "
        "bf16, eager train_step under FlatDDP (masked loss, clip 1.0, FusedAdamW)")
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=a.base_ch, lstm_layers=1, use_skip_lstm=True, use_attention=False).to(dev).train()
    opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    ddp = U.FlatDDP(model, opt.flat)
    data = U.SyntheticSequences(a.batch, a.seq, a.size, a.size, seed=1, kind="uniform", device=dev)

    def round_ms(sync_bn: bool) -> float:
        ddp.sync_bn = sync_bn
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss, _ = U.train_step(model, opt, data.x, data.y, data.mask, True, ddp)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(loss)), float(loss)
        return dt / a.steps * 1e3

    # what the switch adds to one step, counted from the launch log
    ddp.sync_bn = True
    ops.LAUNCH_LOG = []
    try:
        U.train_step(model, opt, data.x, data.y, data.mask, True, ddp)
        torch.cuda.synchronize()
        log = list(ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
    coll = [e for e in log if e[0] == "collective"]
    say(f"per step with the switch on: {sum(1 for e in log if e[0] == 'syncbn')} extra launches, {len(coll)} all-reduces "
        f"({sum(1 for e in coll if e[1] == 'bn_stats')} forward, {sum(1 for e in coll if e[1] == 'bn_bwd_sums')} backward), "
        f"{sum(e[2] for e in coll)} payload bytes in all, largest {max(e[2] for e in coll)} bytes (f64)")

    arms = {"SyncBatchNorm off": False, "SyncBatchNorm on": True}
    times = {k: [] for k in arms}
    for r in range(2 + a.rounds):
        for name, on in arms.items():
            t = round_ms(on)
            if r >= 2:
                times[name].append(t)
    say(f"  {'arm':20s} {'ms/step':>9s} {'min':>8s} {'max':>8s} {'frames/s':>10s}   ({a.rounds} timed rounds of {a.steps} steps per arm, "
        "alternating, after 2 warm-up rounds each)")
    for name, ts in times.items():
        med = statistics.median(ts)
        say(f"  {name:20s} {med:9.2f} {min(ts):8.2f} {max(ts):8.2f} {a.batch * a.seq / med * 1e3:10.0f}")
    off, on = (statistics.median(times[k]) for k in arms)
    spread = max(max(v) - min(v) for v in times.values())
    say(f"  on / off = {on / off:.3f} (median ms/step), difference {on - off:+.2f} ms/step; largest min - max spread of an arm {spread:.2f} ms/step")
    say("  (one rank: the collectives move no data; the cost of the exchange at N > 1 ranks is NOT measured here)")
    say()
    ddp.remove_hooks()
finally:
    dist.destroy_process_group()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
