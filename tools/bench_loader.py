#!/usr/bin/env python3
"""A/B of the two ways an epoch gets its batches, on a synthetic ``.npz`` in the reference's format (N sequences of
T frames of 2 x H x W, written to a temporary directory):

    host    torch.utils.data.DataLoader(dataset, batch_size, shuffle=True, pin_memory=True)      (main.py:245, num_workers=0)
    device  DeviceSequenceLoader(dataset, batch_size, shuffle=True)                              (raw data resident on the GPU)

Both arms run ``train_one_epoch`` over the SAME model and FusedAdamW (the arms alternate epoch by epoch inside one process, so
clock, allocator and cache state are shared); an epoch is timed with a host clock around it -- ``train_one_epoch`` ends in a
device-to-host read of the epoch's sums, so the clock covers the device work.  Two warm-up epochs per arm, then ``--epochs``
timed ones per arm.  Also timed: the gather kernel alone (cold caches: a 1 GiB fill before every launch, HIP events) against
its algorithmic bytes ((C + 1) * 4 read + (C + 2) * 4 written per pixel), the one-off upload of the raw arrays, and the
training step alone on one resident batch (what ``bench.py`` times: the floor for both arms).

``--augment`` times the augmenting gather kernel (``uclstm_dataset_gather_augment``) alone instead, same protocol (cold caches, HIP
events, ``--kernel-rounds`` rounds, the arms alternating inside a round), at the same two shapes: codes without t, codes with t
(through the LDS tile), and a crop to half the frame size (128 -> 64 at the second shape) with all eight codes -- each against the
plain gather kernel writing the same OUTPUT bytes in the same run.

``--sprites`` times the moving-sprite render kernel (``uclstm_sprites_render``) alone, same protocol, against the plain gather
kernel writing the same OUTPUT shape in the same run (both write 16 B per pixel; the gather also reads 12), with and without the
optional raw planes; then an epoch of ``train_one_epoch`` fed by ``render_sprites_host`` plus a pinned host-to-device copy per
batch against one fed by ``DeviceSpriteLoader`` (same model, the arms alternating epoch by epoch).

``--vector`` times the vector-target gather kernel (``uclstm_dataset_gather_vec``) alone, same protocol, in A/B/A order inside a
round: the scalar augmenting kernel (the yardstick), the new kernel at ``Cy = 1`` (the same bytes), the new kernel at ``Cy = 3``
(44 B per pixel instead of 28: compared by achieved bandwidth), and the scalar kernel again -- the distance between the two runs of
the yardstick is the spread the others are read against.  Full frames, all eight codes.

    python tools/bench_loader.py [--epochs 3] [--out profiles/device_loader_ab.txt]
    python tools/bench_loader.py --augment [--out profiles/device_loader_augment_ab.txt]
    python tools/bench_loader.py --sprites [--out profiles/sprites_ab.txt]
    python tools/bench_loader.py --vector [--out profiles/vector_targets_ab.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402
from unet_convlstm_amd import engine as E   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=3, help="timed epochs per arm (>= 3)")
ap.add_argument("--n", type=int, default=256, help="sequences in the synthetic dataset")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--base-ch", type=int, default=64)
ap.add_argument("--shapes", default="20x64,12x128", help="comma-separated TxS: T frames of 2 x S x S")
ap.add_argument("--kernel-rounds", type=int, default=9)
ap.add_argument("--augment", action="store_true", help="time the augmenting gather kernel against the plain one, nothing else")
ap.add_argument("--sprites", action="store_true", help="time the sprite render kernel against the plain gather kernel, and an epoch "
                "fed by the host mirror against one fed by DeviceSpriteLoader")
ap.add_argument("--vector", action="store_true", help="time the vector-target gather kernel against the scalar augmenting kernel (A/B/A)")
ap.add_argument("--vector-transform", default="asinh", choices=["asinh", "signed_log", "none"],
                help="target transform of the --vector arms ('none' separates the traffic from the per-pixel arithmetic)")
ap.add_argument("--out", default=None, help="also append the table to this file")
a = ap.parse_args()
if a.epochs < 3:
    ap.error("--epochs must be at least 3")
if not torch.cuda.is_available():
    sys.exit("bench_loader: needs a GPU (no CPU fallback: a timing taken elsewhere says nothing)")
dev = torch.device("cuda", 0)
lines = []


def say(msg=""):
    print(msg, flush=True)
    lines.append(msg)


def write_npz(path, n, T, S, seed=0):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, T, 2, S, S), dtype=np.float32) * 30).astype(np.float32)
    X[X < 6] = 0.0
    Y = (np.tanh(X[:, :, :1] / 15.0 - 1.0) * 4.0 + rng.standard_normal((n, T, 1, S, S), dtype=np.float32) * 0.5).astype(np.float32)
    np.savez(path, X=X, Y=Y)


def epoch_seconds(model, loader, opt, ds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = U.train_one_epoch(model, loader, opt, dev, ds, use_mask=True)
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in out), out
    return time.perf_counter() - t0


def kernel_alone(ds, loader, T, S):
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1))[:a.batch].to(dev)
    out = tuple(torch.empty((a.batch, T, c, S, S), device=dev) for c in (2, 1, 1))
    st = torch.cuda.current_stream()
    ts = []
    for r in range(a.kernel_rounds + 1):
        flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        E._gather_transform(ds, loader.x_all, loader.y_all, idx, a.batch, out)
        e1.record(st)
        torch.cuda.synchronize()
        if r:                                   # round 0 warms up (code-object load)
            ts.append(e0.elapsed_time(e1) * 1e3)
    nbytes = a.batch * T * S * S * (3 * 4 + 4 * 4)
    med = statistics.median(ts)
    say(f"  gather kernel alone, cold caches, batch {a.batch}: median {med:.1f} us (min {min(ts):.1f}, max {max(ts):.1f}, "
        f"{a.kernel_rounds} rounds); {nbytes / 1e6:.1f} MB algorithmic (28 B/pixel) -> {nbytes / med / 1e3:.0f} GB/s")
    del flush


def augment_kernel(T, S, tmp):
    """The augmenting kernel against the plain one at equal output bytes.  The raw arrays are random device tensors (the dataset
    object only supplies the constants of the transform); every launch follows a 1 GiB fill, the arms alternate inside a round."""
    path = os.path.join(tmp, f"consts_{T}x{S}.npz")
    write_npz(path, 4, T, S)
    ds = U.NPZSequenceDataset(path)
    g = torch.Generator(device=dev).manual_seed(0)
    h = S // 2

    def raw(s):
        x = torch.rand((a.n, T, 2, s, s), device=dev, generator=g) * 30
        return x * (x >= 6), torch.randn((a.n, T, 1, s, s), device=dev, generator=g) * 2

    full, half = raw(S), raw(h)
    idx = torch.randperm(a.n, generator=torch.Generator().manual_seed(1))[:a.batch].to(dev)
    cg = torch.Generator().manual_seed(2)

    def table(codes, span):
        t = torch.zeros((a.batch, 4), dtype=torch.int32)
        t[:, 0] = torch.tensor(codes)[torch.randint(0, len(codes), (a.batch,), generator=cg)]
        if span:
            t[:, 1:3] = torch.randint(0, span // 4 + 1, (a.batch, 2), generator=cg).int() * 4
        return t.to(dev)

    out_full = tuple(torch.empty((a.batch, T, c, S, S), device=dev) for c in (2, 1, 1))
    out_half = tuple(torch.empty((a.batch, T, c, h, h), device=dev) for c in (2, 1, 1))
    tabs = {"no t": table((0, 1, 2, 3), 0), "t": table((4, 5, 6, 7), 0), "crop": table(tuple(range(8)), S - h)}
    arms = {
        f"plain {S}x{S}": lambda: E._gather_transform(ds, *full, idx, a.batch, out_full),
        f"augment {S}x{S}, codes 0-3": lambda: E._gather_augment(ds, *full, idx, tabs["no t"], a.batch, (T, S, S), 3, out_full),
        f"augment {S}x{S}, codes 4-7": lambda: E._gather_augment(ds, *full, idx, tabs["t"], a.batch, (T, S, S), 3, out_full),
        f"plain {h}x{h}": lambda: E._gather_transform(ds, *half, idx, a.batch, out_half),
        f"augment {S} -> {h} crop, codes 0-7": lambda: E._gather_augment(ds, *full, idx, tabs["crop"], a.batch, (T, h, h), 3, out_half),
    }
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream()
    ts = {k: [] for k in arms}
    for r in range(a.kernel_rounds + 1):
        for name, launch in arms.items():
            flush.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            launch()
            e1.record(st)
            torch.cuda.synchronize()
            if r:                               # round 0 warms up (code-object load)
                ts[name].append(e0.elapsed_time(e1) * 1e3)
    say(f"shape: T = {T}, 2 x {S} x {S}, batch {a.batch} of {a.n} resident sequences; cold caches, {a.kernel_rounds} rounds, us")
    say(f"  {'arm':38s} {'median':>8s} {'min':>8s} {'max':>8s} {'GB/s':>7s}   against the plain kernel at the same output bytes")
    base = None
    for name, v in ts.items():
        med = statistics.median(v)
        side = h if (f"{h}x{h}" in name or "crop" in name) else S
        nbytes = a.batch * T * side * side * 28                      # 12 B read + 16 B written per output pixel
        if name.startswith("plain"):
            base, note = v, "the yardstick"
        else:
            bm = statistics.median(base)
            where = "inside" if min(base) <= med <= max(base) else ("below" if med < min(base) else "above")
            note = f"{med / bm:.3f} x its median; {where} its min-max spread [{min(base):.1f}, {max(base):.1f}]"
        say(f"  {name:38s} {med:8.1f} {min(v):8.1f} {max(v):8.1f} {nbytes / med / 1e3:7.0f}   {note}")
    say()
    del flush


def vector_kernel(T, S, tmp):
    """uclstm_dataset_gather_vec against uclstm_dataset_gather_augment, the yardstick, which runs first AND last in every round.
    Random device tensors as raw arrays (the dataset objects only supply constants and the channel map); every launch follows a
    1 GiB fill."""
    rng = np.random.default_rng(0)
    path1, path3 = os.path.join(tmp, f"consts1_{T}x{S}.npz"), os.path.join(tmp, f"consts3_{T}x{S}.npz")
    write_npz(path1, 4, T, S)
    X = (rng.random((4, T, 2, S, S), dtype=np.float32) * 30).astype(np.float32)
    np.savez(path3, X=X, Y=(rng.standard_normal((4, T, 3, S, S), dtype=np.float32) * np.float32([9, 9, 2]).reshape(1, 1, 3, 1, 1)))
    tr = None if a.vector_transform == "none" else a.vector_transform
    ds = U.NPZSequenceDataset(path1, y_transform=tr)
    ds1 = U.VectorNPZDataset(path1, (None,), min_y=ds.min_vel, max_y=ds.max_vel, y_transform=tr)
    ds3 = U.VectorNPZDataset(path3, ("+w", "-h", None), tie_horizontal=True, y_transform=tr)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((a.n, T, 2, S, S), device=dev, generator=g) * 30
    x = x * (x >= 6)
    y3 = torch.randn((a.n, T, 3, S, S), device=dev, generator=g) * 2
    y1 = y3[:, :, :1].contiguous()
    idx = torch.randperm(a.n, generator=torch.Generator().manual_seed(1))[:a.batch].to(dev)
    tab = torch.zeros((a.batch, 4), dtype=torch.int32)
    tab[:, 0] = torch.randint(0, 8, (a.batch,), generator=torch.Generator().manual_seed(2))
    tab = tab.to(dev)
    out1 = tuple(torch.empty((a.batch, T, c, S, S), device=dev) for c in (2, 1, 1))
    out3 = tuple(torch.empty((a.batch, T, c, S, S), device=dev) for c in (2, 3, 1))
    arms = {
        "scalar augment (A)": (lambda: E._gather_augment(ds, x, y1, idx, tab, a.batch, (T, S, S), 3, out1), 28),
        "vector, Cy = 1": (lambda: E._gather_vec(ds1, x, y1, idx, tab, a.batch, (T, S, S), 3, out1), 28),
        "vector, Cy = 3": (lambda: E._gather_vec(ds3, x, y3, idx, tab, a.batch, (T, S, S), 3, out3), 44),
        "scalar augment (A again)": (lambda: E._gather_augment(ds, x, y1, idx, tab, a.batch, (T, S, S), 3, out1), 28),
    }
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream()
    ts = {k: [] for k in arms}
    for r in range(a.kernel_rounds + 1):
        for name, (launch, _) in arms.items():
            flush.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            launch()
            e1.record(st)
            torch.cuda.synchronize()
            if r:                               # round 0 warms up (code-object load)
                ts[name].append(e0.elapsed_time(e1) * 1e3)
    del flush
    px = a.batch * T * S * S
    base, again = ts["scalar augment (A)"], ts["scalar augment (A again)"]
    bm, am = statistics.median(base), statistics.median(again)
    lo, hi = min(base + again), max(base + again)
    say(f"shape: T = {T}, 2 x {S} x {S}, batch {a.batch} of {a.n} resident sequences, all eight codes, transform {a.vector_transform}; "
        f"cold caches, {a.kernel_rounds} rounds, us")
    say(f"  {'arm':26s} {'median':>8s} {'min':>8s} {'max':>8s} {'B/px':>5s} {'GB/s':>7s}   against the yardstick (medians {bm:.1f} and {am:.1f}, "
        f"A-to-A {abs(am - bm) / bm * 100:.1f} %, min-max of both runs [{lo:.1f}, {hi:.1f}])")
    gbase = px * 28 / ((bm + am) / 2) / 1e3
    for name, v in ts.items():
        med, bpp = statistics.median(v), arms[name][1]
        gbs = px * bpp / med / 1e3
        if name.startswith("scalar"):
            note = "the yardstick"
        elif bpp == 28:
            where = "inside" if lo <= med <= hi else ("below" if med < lo else "above")
            note = f"{med / ((bm + am) / 2):.3f} x the yardstick's median; {where} its min-max spread"
        else:
            note = f"{gbs / gbase:.3f} x the yardstick's achieved bandwidth ({gbase:.0f} GB/s)"
        say(f"  {name:26s} {med:8.1f} {min(v):8.1f} {max(v):8.1f} {bpp:5d} {gbs:7.0f}   {note}")
    say()


class HostSpriteLoader:
    """The host way to the same batches: per batch the table is drawn, ``render_sprites_host`` renders it in numpy, (x, y, mask)
    are assembled in pinned memory and copied to the device."""

    def __init__(self, bank, batch, steps, T, S, seed):
        self.bank, self.batch, self.steps, self.T, self.S = bank, batch, steps, T, S
        self.g = torch.Generator().manual_seed(seed)

    def __len__(self):
        return self.steps

    def __iter__(self):
        K, gh, gw = self.bank.shape
        for _ in range(self.steps):
            tab = E.epoch_sprites(self.batch, 2, K, self.S, self.S, gh, gw, 5, self.g)
            data = torch.from_numpy(E.render_sprites_host(self.bank, tab, self.T, self.S, self.S))
            frame, vmap = data[:, :, 0:1], data[:, :, 1:2]
            host = (frame.expand(-1, -1, 2, -1, -1).contiguous().pin_memory(), (vmap / 5.0).pin_memory(),
                    (frame > 0).float().pin_memory())
            yield tuple(t.to(dev, non_blocking=True) for t in host)


def sprites(T, S, tmp):
    """The render kernel against the plain gather kernel at equal output shape (cold caches, the arms alternating inside a round),
    then the two ways to feed an epoch."""
    path = os.path.join(tmp, f"consts_{T}x{S}.npz")
    write_npz(path, 4, T, S)
    ds = U.NPZSequenceDataset(path)
    g = torch.Generator(device=dev).manual_seed(0)
    x_all = torch.rand((a.n, T, 2, S, S), device=dev, generator=g) * 30
    y_all = torch.randn((a.n, T, 1, S, S), device=dev, generator=g) * 2
    idx = torch.randperm(a.n, generator=torch.Generator().manual_seed(1))[:a.batch].to(dev)
    bank_host = U.procedural_glyphs(64, 28, seed=0)
    bank = torch.from_numpy(bank_host).to(dev)
    table = torch.from_numpy(E.epoch_sprites(a.batch, 2, 64, S, S, 28, 28, 5, torch.Generator().manual_seed(2))).to(dev)
    out = tuple(torch.empty((a.batch, T, c, S, S), device=dev) for c in (2, 1, 1))
    raw = torch.empty((a.batch, T, 2, S, S), device=dev)
    arms = {
        "plain gather": (lambda: E._gather_transform(ds, x_all, y_all, idx, a.batch, out), 28, 16),
        "sprites render": (lambda: E._render_sprites(bank, table, a.batch, (T, 2, S, S), 5.0, out), 16, 16),
        "sprites render + raw planes": (lambda: E._render_sprites(bank, table, a.batch, (T, 2, S, S), 5.0, out, raw), 24, 24),
    }
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream()
    ts = {k: [] for k in arms}
    for r in range(a.kernel_rounds + 1):
        for name, (launch, _, _) in arms.items():
            flush.fill_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            launch()
            e1.record(st)
            torch.cuda.synchronize()
            if r:                               # round 0 warms up (code-object load)
                ts[name].append(e0.elapsed_time(e1) * 1e3)
    del flush
    px = a.batch * T * S * S
    say(f"shape: [{a.batch},{T},2,{S},{S}], 2 sprites of 28 x 28; cold caches, {a.kernel_rounds} rounds, us")
    say(f"  {'arm':30s} {'median':>8s} {'min':>8s} {'max':>8s} {'MB moved':>9s} {'TB/s':>6s} {'MB written':>11s} {'TB/s':>6s}   against the plain gather kernel")
    base = ts["plain gather"]
    for name, v in ts.items():
        med, (_, moved, written) = statistics.median(v), arms[name]
        if name == "plain gather":
            note = "the yardstick"
        else:
            where = "inside" if min(base) <= med <= max(base) else ("below" if med < min(base) else "above")
            note = f"{med / statistics.median(base):.3f} x its median; {where} its min-max spread [{min(base):.1f}, {max(base):.1f}]"
        say(f"  {name:30s} {med:8.1f} {min(v):8.1f} {max(v):8.1f} {px * moved / 1e6:9.1f} {px * moved / med / 1e6:6.2f} "
            f"{px * written / 1e6:11.1f} {px * written / med / 1e6:6.2f}   {note}")
    del x_all, y_all
    # ---- an epoch fed either way
    steps = a.n // a.batch
    device_loader = U.DeviceSpriteLoader(bank_host, a.batch, steps, T=T, H=S, W=S, generator=torch.Generator().manual_seed(7))
    host_loader = HostSpriteLoader(bank_host, a.batch, steps, T, S, 7)
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=a.base_ch, lstm_layers=1, use_skip_lstm=True, use_attention=False).to(dev)
    opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    loaders = {"render_sprites_host + H2D": host_loader, "DeviceSpriteLoader": device_loader}
    times = {k: [] for k in loaders}
    for r in range(2 + a.epochs):
        for name, loader in loaders.items():
            t = epoch_seconds(model, loader, opt, device_loader)
            if r >= 2:
                times[name].append(t)
    say(f"  epochs of {steps} steps, base_ch {a.base_ch}, bf16 ({a.epochs} timed epochs per arm, alternating, after 2 warm-up epochs each)")
    say(f"  {'arm':30s} {'ms/step':>9s} {'min':>8s} {'max':>8s} {'frames/s':>10s}")
    for name, v in times.items():
        per = [t / steps * 1e3 for t in v]
        med = statistics.median(per)
        say(f"  {name:30s} {med:9.2f} {min(per):8.2f} {max(per):8.2f} {a.batch * T / med * 1e3:10.0f}")
    h, d = (statistics.median(times[k]) for k in loaders)
    say(f"  device arm / host arm = {d / h:.3f} (median epoch time)")
    step_alone(model, opt, device_loader)
    say()


def step_alone(model, opt, loader):
    x, y, m = next(iter(loader))
    for _ in range(3):
        U.train_step(model, opt, x, y, m, True)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(8):
            U.train_step(model, opt, x, y, m, True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 8 * 1e3)
    say(f"  training step alone on one resident batch (the bench.py measurement, 8 steps x 3): median {statistics.median(ts):.2f} ms "
        f"(min {min(ts):.2f}, max {max(ts):.2f})")


def one_shape(T, S, tmp):
    path = os.path.join(tmp, f"bench_{T}x{S}.npz")
    write_npz(path, a.n, T, S)
    ds = U.NPZSequenceDataset(path)
    say(f"shape: N = {a.n}, T = {T}, 2 x {S} x {S}, batch {a.batch} ({a.n // a.batch} steps per epoch), base_ch {a.base_ch}, bf16; "
        f"raw arrays {(ds.X.nbytes + ds.Y.nbytes) / 1e6:.0f} MB")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    device_loader = U.DeviceSequenceLoader(ds, a.batch, shuffle=True, generator=torch.Generator().manual_seed(7), drop_last=True)
    torch.cuda.synchronize()
    up = time.perf_counter() - t0
    say(f"  one-off upload of the raw arrays (pageable host memory): {up * 1e3:.1f} ms "
        f"({(ds.X.nbytes + ds.Y.nbytes) / up / 1e9:.1f} GB/s)")
    host_loader = torch.utils.data.DataLoader(ds, batch_size=a.batch, shuffle=True, pin_memory=True, drop_last=True,
                                              generator=torch.Generator().manual_seed(7))
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=a.base_ch, lstm_layers=1, use_skip_lstm=True, use_attention=False).to(dev)
    opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    arms = {"host DataLoader": host_loader, "DeviceSequenceLoader": device_loader}
    times = {k: [] for k in arms}
    for r in range(2 + a.epochs):
        for name, loader in arms.items():
            t = epoch_seconds(model, loader, opt, ds)
            if r >= 2:
                times[name].append(t)
    steps = a.n // a.batch
    say(f"  {'arm':22s} {'ms/step':>9s} {'min':>8s} {'max':>8s} {'frames/s':>10s}   ({a.epochs} timed epochs per arm, alternating, after 2 warm-up epochs each)")
    for name, ts in times.items():
        per = [t / steps * 1e3 for t in ts]
        med = statistics.median(per)
        say(f"  {name:22s} {med:9.2f} {min(per):8.2f} {max(per):8.2f} {a.batch * T / med * 1e3:10.0f}")
    h, d = (statistics.median(times[k]) for k in arms)
    spread = max(max(v) - min(v) for v in times.values()) / steps * 1e3
    say(f"  device arm / host arm = {d / h:.3f} (median epoch time); largest min - max spread of an arm {spread:.2f} ms/step")
    step_alone(model, opt, device_loader)
    kernel_alone(ds, device_loader, T, S)
    say()


with tempfile.TemporaryDirectory() as tmp:
    say(f"tools/bench_loader.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    torch.zeros(1 << 20, device=dev).sum().item()          # the HIP context and the allocator exist before the first timed upload
    for shape in a.shapes.split(","):
        T, S = (int(v) for v in shape.split("x"))
        if a.vector:
            vector_kernel(T, S, tmp)
        elif a.augment:
            augment_kernel(T, S, tmp)
        elif a.sprites:
            sprites(T, S, tmp)
        else:
            one_shape(T, S, tmp)
        torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
