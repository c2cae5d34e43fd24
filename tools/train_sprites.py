#!/usr/bin/env python3
"""Train ``TemporalUNetDualView`` on Moving-MNIST sequences rendered on the GPU (``DeviceSpriteLoader``): every epoch is
``--steps`` fresh batches, one kernel launch each; a ``fixed=True`` loader is the validation set.  Prints the
``train_one_epoch`` and ``evaluate`` tuples ``(loss, mae, rmse, mean error)`` per epoch, errors in pixels per frame.

The glyphs are MNIST digits when ``--idx`` names an IDX image file the user already has (``train-images-idx3-ubyte[.gz]``),
the built-in procedural bank otherwise; nothing is downloaded.

``--burn-in K`` gives the first K frames of every sequence the weight 0 in the training and the validation loss
(``WeightedLossSpec.burn_in``: a ConvLSTM has no history at t = 0); the error columns still cover all frames.

``--monitor`` attaches a ``StepMonitor`` with the model's parameter names (``FusedAdamW.attach_monitor``, one record per epoch: the
update columns are the change over the epoch) and prints its ``report()`` after every epoch.

    python tools/train_sprites.py [--epochs 4] [--steps 16] [--batch 32] [--burn-in 0] [--monitor] [--idx PATH] [--out profiles/sprites_train.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_convlstm_amd as U   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=4)
ap.add_argument("--steps", type=int, default=16, help="batches per training epoch")
ap.add_argument("--val-steps", type=int, default=4)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--sprites", type=int, default=2)
ap.add_argument("--base-ch", type=int, default=64)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--burn-in", type=int, default=0, help="frames at the start of every sequence that do not count in the loss")
ap.add_argument("--monitor", action="store_true", help="per-tensor gradient / weight / update statistics, reported once per epoch")
ap.add_argument("--idx", default=None, help="an MNIST IDX image file; default: procedural glyphs")
ap.add_argument("--out", default=None, help="also append the log to this file")
a = ap.parse_args()
if not 0 <= a.burn_in < a.frames:
    sys.exit(f"train_sprites: --burn-in must be in 0 .. {a.frames - 1}")
if not torch.cuda.is_available():
    sys.exit("train_sprites: needs a GPU (this package has no CPU path)")
dev = torch.device("cuda", 0)
lines = []


def say(msg=""):
    print(msg, flush=True)
    lines.append(msg)


bank = U.load_idx_images(a.idx) if a.idx else U.procedural_glyphs(256, 28, seed=a.seed)
shape = dict(T=a.frames, H=a.size, W=a.size, num_sprites=a.sprites)
train = U.DeviceSpriteLoader(bank, a.batch, a.steps, generator=torch.Generator().manual_seed(a.seed + 1), **shape)
val = U.DeviceSpriteLoader(bank, a.batch, a.val_steps, generator=torch.Generator().manual_seed(a.seed + 2), fixed=True, **shape)
torch.manual_seed(a.seed)
model = U.TemporalUNetDualView(1, 1, base_ch=a.base_ch, lstm_layers=1, use_skip_lstm=True, use_attention=False).to(dev)
opt = U.FusedAdamW(model.parameters(), lr=a.lr, weight_decay=1e-4, max_grad_norm=1.0)
monitor = opt.attach_monitor(every=a.steps, history=max(1, a.epochs), names=model.named_parameters()) if a.monitor else None
loss = U.WeightedLossSpec.burn_in(a.frames, a.burn_in) if a.burn_in else None
say(f"tools/train_sprites.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
say(f"{'MNIST ' + os.path.basename(a.idx) if a.idx else 'procedural'} bank of {len(bank)} glyphs; [{a.batch},{a.frames},2,{a.size},{a.size}], "
    f"{a.sprites} sprites, base_ch {a.base_ch}, bf16; {a.steps} fresh batches per epoch, {a.val_steps} fixed validation batches"
    + (f"; the loss skips the first {a.burn_in} frames" if a.burn_in else ""))
say(f"{'epoch':>5s}  {'train loss':>10s} {'mae':>7s} {'rmse':>7s} {'bias':>8s}   {'val loss':>10s} {'mae':>7s} {'rmse':>7s} {'bias':>8s}   {'s':>6s}")
for epoch in range(a.epochs):
    t0 = time.perf_counter()
    tr = U.train_one_epoch(model, train, opt, dev, train, use_mask=True, loss=loss)
    ev = U.evaluate(model, val, dev, val, use_mask=True, loss=loss)
    say(f"{epoch:5d}  {tr[0]:10.5f} {tr[1]:7.4f} {tr[2]:7.4f} {tr[3]:8.4f}   {ev[0]:10.5f} {ev[1]:7.4f} {ev[2]:7.4f} {ev[3]:8.4f}   "
        f"{time.perf_counter() - t0:6.2f}")
    if monitor is not None:
        say(monitor.report())
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
