#!/usr/bin/env python3
"""First record of PretrainedTemporalUNet on the HIP path (profiles/resnet_step.txt).

  * one ``train_step`` of the reference's shipped configuration: B = 32, T = 20, 64 x 64, lstm_layers = 2, frozen encoder, bf16,
    FusedAdamW with the clip fused -- HIP events around every step, median / min / max over --steps steps after --warmup;
  * every kernel of csrc/resnet.hip alone at the shapes that step gives it, with cold caches (a 1 GiB fill before every launch, so
    nothing is served from the 256 MB memory-side cache): median microseconds and achieved TB/s against ALGORITHMIC bytes (every
    operand read once, every result written once).

There is nothing to compare with: the parent cannot run this model and the eager smp path cannot run here.

``--unfreeze all`` (or ``layer3,layer4`` ...; profiles/resnet_unfrozen_step.txt): after the frozen step, the same step with that part of
the encoder trainable (``model.unfreeze_encoder``, two optimiser groups, the encoder at lr / 10), the peak memory of both, the share
of the step that the backward kernels of csrc/resnet_bwd.hip take (HIP events around each of their launches in a few further steps), and
those kernels alone at the step's shapes like the ones above.

``--rollout`` (profiles/resnet_rollout.txt) measures frame-by-frame inference instead and does nothing else: the shipped
configuration (lstm_layers = 2) at B = 1, T = --frames, for each of --rollout-sizes (64 and 256), frames/s of one T-frame sequence
between HIP events -- median, min and max of --iters sequences after two untimed ones --
  (a) the reference's method on this code (test.py:305-310): ``model(x[:, :t])`` for t = 1 .. T under no_grad, T (T + 1) / 2 frames of work;
  (b) ``PretrainedStreamingPredictor`` eager;  (c) with HIP graphs;  (d) as (c) with ``ops.GROUP_LSTM = False``: every cell step a
  launch of its own, what the group launches of ``ops.convlstm_tick`` replace.  (c) and (d) are timed alternately.

    python tools/bench_resnet.py [--steps 10] [--warmup 3] [--batch 32] [--frames 20] [--unfreeze STAGES] [--out FILE]
    python tools/bench_resnet.py --rollout [--frames 20] [--rollout-sizes 64,256] [--iters 7] [--out profiles/resnet_rollout.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd import ops   # noqa: E402

L = U._lib
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--unfreeze", default=None, help="all, or a comma-separated list of stem, layer1 .. layer4")
ap.add_argument("--rollout", action="store_true", help="measure frame-by-frame inference (B = 1) and nothing else")
ap.add_argument("--rollout-sizes", default="64,256")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("a HIP device is required (this package has no CPU path)")
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def rollout_record():
    T = a.frames
    say(f"# PretrainedTemporalUNet(lstm_layers=2), evaluation mode, bf16, B=1 T={T}, {torch.cuda.get_device_name(0)}")
    say(f"# frames/s of one {T}-frame sequence between HIP events: median (min .. max) of {a.iters} sequences after 2 untimed ones")
    torch.manual_seed(0)
    model = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=2).to(dev).eval()

    def timed_once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return T / e0.elapsed_time(e1) * 1e3, out

    def line(tag, what, fps):
        fps = sorted(fps)
        say(f"{tag} {what:58s} {fps[len(fps) // 2]:9.1f} frames/s ({fps[0]:.1f} .. {fps[-1]:.1f})   {1e3 / fps[len(fps) // 2]:7.3f} ms/frame")
        return fps[len(fps) // 2]

    for size in (int(v) for v in a.rollout_sizes.split(",")):
        x = torch.randn(1, T, 2, size, size, generator=torch.Generator().manual_seed(size)).to(dev)
        say()
        say(f"## {size} x {size}")

        def prefixes():
            with torch.no_grad():
                return torch.cat([model(x[:, :t])[0][:, -1:] for t in range(1, T + 1)], dim=1)

        def rolled(pred, group):
            def fn():
                ops.GROUP_LSTM = group
                try:
                    pred.new_sequence()
                    return pred.rollout(x)
                finally:
                    ops.GROUP_LSTM = True
            return fn

        eager = rolled(U.PretrainedStreamingPredictor(model, use_graph=False), True)
        graph = rolled(U.PretrainedStreamingPredictor(model, use_graph=True), True)
        single = rolled(U.PretrainedStreamingPredictor(model, use_graph=True), False)
        runs = {"a": prefixes, "b": eager, "c": graph, "d": single}
        outs = {}
        for k, fn in runs.items():
            for _ in range(2):
                outs[k] = fn()
        torch.cuda.synchronize()
        fps = {k: [] for k in runs}
        for _ in range(a.iters):
            for k in ("a", "b", "c", "d", ):          # (c) and (d) alternate: neighbours in time see the same machine
                fps[k].append(timed_once(runs[k])[0])
        med = {}
        med["a"] = line("(a)", f"prefix loop model(x[:, :t]), {T * (T + 1) // 2} frames of work", fps["a"])
        med["b"] = line("(b)", "PretrainedStreamingPredictor, eager", fps["b"])
        med["c"] = line("(c)", "PretrainedStreamingPredictor, HIP graphs", fps["c"])
        med["d"] = line("(d)", "as (c) with ops.GROUP_LSTM = False (every cell step alone)", fps["d"])
        rel = lambda k: float((outs["c"] - outs[k]).norm() / outs[k].norm())
        say(f"(c) / (d) = {med['c'] / med['d']:.3f}, (c) / (a) = {med['c'] / med['a']:.1f}; rel-L2 of the {T} predictions of (c) against those of "
            f"(a) {rel('a'):.2e}, (b) {rel('b'):.2e}, (d) {rel('d'):.2e}")
        ops.LAUNCH_LOG = log = []
        eager()
        ops.LAUNCH_LOG = None
        ticks = [e for e in log if e[0] == "tick"]
        per_frame = len(ticks) // T
        say(f"launches of ops.convlstm_tick per frame (two layers): {ticks[-per_frame:]}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if a.rollout:
    rollout_record()
    raise SystemExit(0)

B, T, HW = a.batch, a.frames, a.size
say(f"# PretrainedTemporalUNet(lstm_layers=2, freeze_encoder=True), bf16, B={B} T={T} {HW}x{HW}, {torch.cuda.get_device_name(0)}")
torch.manual_seed(0)
model = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=2).to(dev).train()
trainable = [p for p in model.parameters() if p.requires_grad]
say(f"# parameters: {sum(p.numel() for p in model.parameters())} ({sum(p.numel() for p in trainable)} trainable)")
opt = U.FusedAdamW(trainable, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
g = torch.Generator().manual_seed(1)
x = torch.randn(B, T, 2, HW, HW, generator=g).to(dev)
y = (torch.randn(B, T, 1, HW, HW, generator=g) * 0.5).to(dev)
mask = (torch.rand(B, T, 1, HW, HW, generator=g) > 0.2).float().to(dev)


def time_steps(model, opt, label):
    """Median / min / max of --steps train_steps after --warmup, and the peak allocated memory of those steps."""
    losses = []
    for _ in range(a.warmup):
        losses.append(U.train_step(model, opt, x, y, mask, True)[0])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ev = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        losses.append(U.train_step(model, opt, x, y, mask, True)[0])
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    say(f"{label}: median {ms[len(ms) // 2]:.2f} ms, min {ms[0]:.2f}, max {ms[-1]:.2f} over {a.steps} steps after {a.warmup} warm-up steps "
        f"({B * T / ms[len(ms) // 2] * 1e3:.0f} frames/s); loss {float(losses[0]):.4f} -> {float(losses[-1]):.4f}; "
        f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    return ms[len(ms) // 2]


time_steps(model, opt, "train_step")
with torch.no_grad():
    model.eval()
    for _ in range(2):
        model(x)
    torch.cuda.synchronize()
    ev = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model(x)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
say(f"eval forward (no_grad): median {ms[len(ms) // 2]:.2f} ms, min {ms[0]:.2f}, max {ms[-1]:.2f}")
del model, opt
torch.cuda.empty_cache()

# ---- the same step with a trainable encoder ---------------------------------------------------
BWD_KINDS = ("maxpool3s2_bwd", "bn_add_relu_bwd_reduce", "bn_add_relu_bwd_apply")
if a.unfreeze:
    stages = "all" if a.unfreeze == "all" else tuple(a.unfreeze.split(","))
    say()
    say(f"# the same step after model.unfreeze_encoder({stages!r}); two optimiser groups, the encoder at lr / 10")
    torch.manual_seed(0)
    model = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=2).to(dev)
    model.unfreeze_encoder(stages).train()
    enc = [p for p in model.encoder.parameters() if p.requires_grad]
    rest = [p for k, p in model.named_parameters() if p.requires_grad and ".encoder." not in k and not k.startswith("encoder.")]
    say(f"# trainable parameters: {sum(p.numel() for p in enc)} of the encoder + {sum(p.numel() for p in rest)}")
    opt = U.FusedAdamW([{"params": enc, "lr": 1e-4}, {"params": rest}], lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, order=model.parameters())
    step_ms = time_steps(model, opt, "train_step (unfrozen)")
    # the share of the new backward kernels: events around each of their launches (and of every other HBM-bound kernel) in three
    # further steps; the step itself is slower with the events in it, so the sum is set against the median above
    ops.PROFILE_HBM = prof = []
    for _ in range(3):
        U.train_step(model, opt, x, y, mask, True)
    torch.cuda.synchronize()
    ops.PROFILE_HBM = None
    tot = {}
    for kind, nbytes, e0, e1, _ in prof:
        t = tot.setdefault(kind, [0.0, 0.0, 0])
        t[0] += e0.elapsed_time(e1) / 3
        t[1] += nbytes / 3
        t[2] += 1
    new_ms = 0.0
    for kind in BWD_KINDS:
        if kind in tot:
            ms_, by, cnt = tot[kind]
            new_ms += ms_
            say(f"in the step: {kind:24s} {cnt // 3:3d} launches {ms_:7.3f} ms per step {by / ms_ / 1e9:6.2f} TB/s (algorithmic bytes, event-timed)")
    say(f"in the step: the kernels of csrc/resnet_bwd.hip take {new_ms:.3f} ms of {step_ms:.2f} ms ({100 * new_ms / step_ms:.1f} %)")
    del model, opt
    torch.cuda.empty_cache()

# ---- the kernels of csrc/resnet.hip alone -----------------------------------------------------
flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
st = torch.cuda.current_stream()
K, S = L.lib, ops._stream()
n = B * T


def timed(fn):
    t = []
    for _ in range(a.iters):
        flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    t.sort()
    return t[len(t) // 2]


def act(*shape):
    return torch.randn(shape, device=dev).to(torch.bfloat16)


def nb(*ts):
    return sum(t.numel() * t.element_size() for t in ts)


def report(name, shape, nbytes, fn):
    t = timed(fn)
    say(f"{name:24s} {shape:28s} {nbytes / 1e6:9.1f} MB {t:9.1f} us {nbytes / t / 1e6:6.2f} TB/s")


say()
say(f"# kernels alone, cold caches, median of {a.iters}: name, shape, algorithmic bytes, time, achieved bandwidth")
h2 = HW // 2
col = torch.empty((n, h2, h2, 104), dtype=torch.bfloat16, device=dev)
report("im2col7x7s2_first", f"[{n},{h2},{h2},104]", nb(x, col),
       lambda: L.check(K.uclstm_im2col7x7s2_first(x.data_ptr(), col.data_ptr(), n, 2, 104, HW, HW, B, 2 * HW * HW, T * 2 * HW * HW, S), "im2col"))
f1 = act(n, h2, h2, 64)
p = torch.empty((n, h2 // 2, h2 // 2, 64), dtype=torch.bfloat16, device=dev)
report("maxpool3s2_fwd", f"[{n},{h2},{h2},64]", nb(f1, p), lambda: L.check(K.uclstm_maxpool3s2_fwd(f1.data_ptr(), p.data_ptr(), n, h2, h2, 64, S), "maxpool"))
for C_, hh in ((64, HW // 4), (128, HW // 8), (512, HW // 32)):
    z, r, o = act(n * hh * hh, C_), act(n * hh * hh, C_), torch.empty((n * hh * hh, C_), dtype=torch.bfloat16, device=dev)
    sc = [torch.rand(C_, device=dev) + 0.5 for _ in range(4)]
    report("bn_add_relu", f"[{n},{hh},{hh},{C_}] both affines", nb(z, r, o),
           lambda: L.check(K.uclstm_bn_add_relu(z.data_ptr(), sc[0].data_ptr(), sc[1].data_ptr(), r.data_ptr(), sc[2].data_ptr(), sc[3].data_ptr(),
                                                o.data_ptr(), n * hh * hh, C_, S), "bn_add_relu"))
for C_, hh in ((32, HW // 2), (512, HW // 32)):
    lo, hi = act(n, hh, hh, C_), act(n, 2 * hh, 2 * hh, C_)
    report("upsample2_fwd", f"[{n},{hh},{hh},{C_}] -> x2", nb(lo, hi), lambda: L.check(K.uclstm_upsample2_fwd(lo.data_ptr(), hi.data_ptr(), n, hh, hh, C_, S), "up"))
    report("upsample2_bwd", f"[{n},{hh},{hh},{C_}] <- x2", nb(lo, hi), lambda: L.check(K.uclstm_upsample2_bwd(hi.data_ptr(), lo.data_ptr(), n, hh, hh, C_, S), "upb"))
ah, w, b_ = act(n, HW, HW, 16), torch.randn(1, 16, 3, 3, device=dev) * 0.1, torch.zeros(1, device=dev)
yh, dy, da = torch.empty((n, 1, HW, HW), device=dev), torch.randn(n, 1, HW, HW, device=dev), torch.empty_like(ah)
dw, db = torch.zeros_like(w), torch.zeros_like(b_)
geom = (n, HW, HW, 16, 16, 1)
report("head3x3_fwd", f"[{n},{HW},{HW},16] -> 1", nb(ah, yh),
       lambda: L.check(K.uclstm_head3x3_fwd(ah.data_ptr(), w.data_ptr(), b_.data_ptr(), yh.data_ptr(), *geom, S), "head_fwd"))
report("head3x3_bwd (da, dw, db)", f"[{n},{HW},{HW},16]", nb(ah, dy, da),
       lambda: L.check(K.uclstm_head3x3_bwd(ah.data_ptr(), w.data_ptr(), dy.data_ptr(), da.data_ptr(), dw.data_ptr(), db.data_ptr(), *geom, S), "head_bwd"))
rows = int(K.uclstm_head3x3_bwd_ordered_rows(n, HW, HW))
part = torch.empty(rows * (16 * 9 + 1), device=dev)
report("head3x3_bwd_ordered", f"[{n},{HW},{HW},16] {rows} rows", nb(ah, dy, da),
       lambda: L.check(K.uclstm_head3x3_bwd_ordered(ah.data_ptr(), w.data_ptr(), dy.data_ptr(), da.data_ptr(), part.data_ptr(), dw.data_ptr(),
                                                    db.data_ptr(), 0, *geom, L.ACT_TYPE_BF16, S), "head_bwd_ordered"))
if a.unfreeze:
    say()
    say(f"# backward kernels of csrc/resnet_bwd.hip alone, cold caches, median of {a.iters}")
    dp = act(n, h2 // 2, h2 // 2, 64)
    dsk, da1 = act(n, h2, h2, 64), torch.empty_like(f1)
    f1.clamp_(min=0)                                    # post-ReLU, as in the model: exact ties at zero
    for name, skip in (("maxpool3s2_bwd + dskip", dsk), ("maxpool3s2_bwd", None)):
        report(name, f"[{n},{h2},{h2},64]", nb(f1, dp, da1) + (nb(dsk) if skip is not None else 0),
               lambda: L.check(K.uclstm_maxpool3s2_bwd(f1.data_ptr(), dp.data_ptr(), None if skip is None else skip.data_ptr(), da1.data_ptr(),
                                                       n, h2, h2, 64, S), "maxpool3s2_bwd"))
    for C_, hh, raff in ((64, HW // 4, False), (128, HW // 8, True), (128, HW // 8, False), (512, HW // 32, True)):
        px = n * hh * hh
        z, r, g_ = act(px, C_), act(px, C_), act(px, C_)
        dz, dr = torch.empty_like(z), torch.empty_like(z)
        par = [torch.rand(C_, device=dev) + 0.5 for _ in range(8)]
        pz = [t.data_ptr() for t in par[:4]]
        pr = [t.data_ptr() for t in par[4:]] if raff else [None] * 4
        sums, rsums = torch.empty((C_, 2), device=dev), torch.empty((C_, 2), device=dev) if raff else None
        prt = torch.empty((int(K.uclstm_bn_add_relu_bwd_rows(px)), C_, 3), device=dev)
        rp = None if rsums is None else rsums.data_ptr()
        what = f"[{n},{hh},{hh},{C_}] {'bn_r' if raff else 'identity'}"
        report("bn_add_relu_bwd_reduce", what, nb(z, r, g_),
               lambda: L.check(K.uclstm_bn_add_relu_bwd_reduce(z.data_ptr(), *pz, r.data_ptr(), *pr, g_.data_ptr(), prt.data_ptr(), sums.data_ptr(), rp,
                                                               px, C_, S), "bn_add_relu_bwd_reduce"))
        report("bn_add_relu_bwd_apply", what, nb(z, r, g_, dz, dr),
               lambda: L.check(K.uclstm_bn_add_relu_bwd_apply(z.data_ptr(), *pz, sums.data_ptr(), r.data_ptr(), *pr, rp, g_.data_ptr(), dz.data_ptr(),
                                                              dr.data_ptr(), px, C_, S), "bn_add_relu_bwd_apply"))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
