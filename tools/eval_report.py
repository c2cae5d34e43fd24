"""Evaluation report of a trained model on the validation split: the flow of the reference's train/get_metrics.py with the
statistics computed on the device (unet_convlstm_amd.evaluate_report) and every path given on the command line.

    python tools/eval_report.py --checkpoint model.pt --npz data.npz [--batch 8] [--use-mask] [--out report.npz] [--plots DIR]
    python tools/eval_report.py --checkpoint model.pt --npz wind.npz --axes "+w,-h,none" [--tie-horizontal] [--out report.npz]
    python tools/eval_report.py --bench            # kernel timing against uclstm_metric_sums, see profiles/eval_report.txt
    python tools/eval_report.py --bench --vector   # uclstm_eval_stats_vec against Cy scalar launches, see profiles/eval_report_vec.txt

The checkpoint is what the reference's training writes: {"config": {...}, "model_state": state_dict}, of model type 'custom'
(TemporalUNetDualView) or 'resnet18' (PretrainedTemporalUNet: lstm_layers from the config or counted in the keys).  --plots
draws the reference's five figures from the report when matplotlib can be imported, after everything that is timed.
--axes: the target is a vector (VectorNPZDataset, one entry per channel: +w, -w, +h, -h or none); the model's head is sized from the
checkpoint's own head weight and the report is VectorEvalReport's: per channel what the scalar report holds (keys ch<c>_*), and
speed / endpoint / direction errors when there is a horizontal pair (keys vector_*).  No figures with --axes.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def flat(report: dict) -> dict:
    """The report as a flat {name: array} mapping for np.savez."""
    out = {}
    for k, v in report.items():
        if isinstance(v, dict):
            out.update({f"{k}_{kk}": np.asarray(vv) for kk, vv in v.items()})
        else:
            out[k] = np.asarray(v)
    return out


def flat_vector(report: dict) -> dict:
    """The dict of VectorEvalReport.result as a flat {name: array} mapping: ch<c>_<key> per channel, vector_<key>, axes."""
    out = {"axes": np.asarray(["none" if a is None else a for a in report["axes"]])}
    for c, ch in enumerate(report["channels"]):
        out.update({f"ch{c}_{k}": v for k, v in flat(ch).items()})
    if report["vector"] is not None:
        out.update({f"vector_{k}": v for k, v in flat(report["vector"]).items()})
    return out


def load_model(U, checkpoint_path, device, vector=False):
    checkpoint = torch.load(checkpoint_path, map_location="cpu")
    cfg = checkpoint.get("config", {})
    model_type = cfg.get("type", "custom")
    print(f"[INFO] Detected Model Type: {model_type}")
    state = checkpoint["model_state"]
    if model_type == "resnet18":
        # train/get_metrics.py:75-79 rebuilds PretrainedTemporalUNet(lstm_layers=2); the layer count is in the config of newer
        # checkpoints and in the keys of every one (lstm.layers.<l>.conv.weight)
        layers = cfg.get("lstm_layers")
        if layers is None:
            layers = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("lstm.layers."))
        model = U.PretrainedTemporalUNet(out_channels=state["head.0.weight"].shape[0], lstm_layers=int(layers),
                                         freeze_encoder=cfg.get("freeze_encoder", True))
        model.load_state_dict(state, strict=True)
        return model.to(device).eval()
    if model_type != "custom":
        raise SystemExit(f"model type {model_type!r} is not supported ('custom': TemporalUNetDualView, 'resnet18': PretrainedTemporalUNet)")
    model = U.TemporalUNetDualView(in_channels_per_sat=1, out_channels=state["outc.conv.weight"].shape[0] if vector else 1, base_ch=cfg.get("base_ch", 64), lstm_layers=1,
                                   use_skip_lstm=cfg.get("use_skip_lstm", True), use_attention=cfg.get("use_attention", False))
    model.load_state_dict(state)
    return model.to(device).eval()


def draw(report: dict, out_dir: str) -> bool:
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception as e:                                           # noqa: BLE001  (any import problem: no figures)
        print(f"[WARNING] matplotlib is not usable ({e}); no figures drawn")
        return False
    os.makedirs(out_dir, exist_ok=True)
    lim = 1.1 * max(abs(report["gt_min"]), abs(report["gt_max"]), abs(report["pred_min"]), abs(report["pred_max"]))
    fig, ax = plt.subplots(figsize=(8, 8))
    ax.scatter(report["scatter_gt"], report["scatter_pred"], c="tab:blue", s=2, alpha=0.3)
    ax.plot([-lim, lim], [-lim, lim], "k--")
    ax.set(xlabel="Ground Truth [m/s]", ylabel="Predicted [m/s]", title="Balanced Scatter Plot", xlim=(-lim, lim), ylim=(-lim, lim))
    ax.grid(True, alpha=0.3)
    fig.savefig(os.path.join(out_dir, "scatter_plot.pdf"))
    plt.close(fig)
    fig, ax = plt.subplots(figsize=(10, 5))
    mae_t = report["per_timestep"]["mae"]
    ax.plot(np.arange(len(mae_t)), mae_t, "o-", color="darkblue", label="MAE [m/s]")
    ax.set(xlabel="Time Step", ylabel="MAE [m/s]", title="Mean Absolute Error over Sequence Time", ylim=(0, 1))
    ax.grid(True, alpha=0.3)
    ax.legend()
    fig.savefig(os.path.join(out_dir, "mae_over_time.pdf"))
    plt.close(fig)
    for name, key, edges, color, title, mu, sd in (
            ("histogram_gt", "hist_gt", "hist_edges", "green", "Ground Truth Distribution", report["gt_mean"], report["gt_std"]),
            ("histogram_pred", "hist_pred", "hist_edges", "orange", "Prediction Distribution", report["pred_mean"], report["pred_std"]),
            ("histogram_error", "hist_err", "err_edges", "red", "Error Distribution (Pred - GT)", report["mean_err"], report["std_err"])):
        e, c = report[edges], report[key].astype(np.float64)
        dens = c / max(c.sum(), 1.0) / np.diff(e)                    # density=True of plt.hist
        fig, ax = plt.subplots(figsize=(8, 6))
        ax.bar(e[:-1], dens, width=np.diff(e), align="edge", color=color, alpha=0.7)
        ax.set(title=f"{title}\n$\\mu={mu:.2f}, \\sigma={sd:.2f}$", xlabel="Error [m/s]" if key == "hist_err" else "Velocity [m/s]",
               ylabel="Density", xlim=(e[0], e[-1]))
        if key == "hist_err":
            ax.axvline(0, color="k", linestyle="--")
        ax.grid(True, alpha=0.3)
        fig.savefig(os.path.join(out_dir, name + ".pdf"))
        plt.close(fig)
    print(f"[INFO] All individual PDFs saved to {out_dir}")
    return True


def run_vector(args, U, device) -> None:
    axes = tuple(None if a.strip().lower() == "none" else a.strip() for a in args.axes.split(","))
    if args.plots:
        raise SystemExit("--plots draws the scalar report's figures; there are none for --axes")
    print(f"[INFO] Loading checkpoint: {args.checkpoint}")
    model = load_model(U, args.checkpoint, device, vector=True)
    full_dataset = U.VectorNPZDataset(args.npz, axes, tie_horizontal=args.tie_horizontal)
    if model.out_channels != full_dataset.Cy:
        raise SystemExit(f"the checkpoint's head has {model.out_channels} outputs, --axes names {full_dataset.Cy} channels")
    n_train = int(0.8 * len(full_dataset))                           # the split of training, same seed
    generator = torch.Generator().manual_seed(42)
    _, val_ds = torch.utils.data.random_split(full_dataset, [n_train, len(full_dataset) - n_train], generator=generator)
    print(f"[INFO] Dataset loaded. Evaluating on VALIDATION set only ({len(val_ds)} sequences)")
    loader = U.DeviceSequenceLoader(val_ds, args.batch)
    t0 = time.perf_counter()
    loss, mae, rmse, me, report = U.evaluate_vector_report(model, loader, device, full_dataset, use_mask=args.use_mask)
    dt = time.perf_counter() - t0
    print("\n" + "=" * 40)
    for c, ch in enumerate(report["channels"]):
        print(f"Channel {c} ({axes[c]}): MAE {ch['mae']:.4f}  RMSE {ch['rmse']:.4f}  Bias {ch['mean_err']:.4f}  Error Std {ch['std_err']:.4f} m/s")
    v = report["vector"]
    if v is not None:
        print(f"Speed MAE:         {v['speed_mae']:.4f} m/s (bias {v['speed_bias']:.4f})")
        print(f"Endpoint Error:    {v['epe_mean']:.4f} m/s (RMS {v['epe_rmse']:.4f}, max {v['epe_max']:.4f})")
        print(f"Direction MAE:     {v['dir_mae']:.2f} deg (bias {v['dir_bias']:.2f}, std {v['dir_std']:.2f}, {int(v['n_dir'])} of {int(v['n'])} pixels)")
    print("=" * 40)
    print(f"[INFO] loss {loss:.6f}; pooled MAE {mae:.4f} RMSE {rmse:.4f}; {len(val_ds)} sequences in {dt:.3f} s")
    if args.out:
        np.savez(args.out, loss=np.float64(loss), **flat_vector(report))
        print(f"[INFO] report written to {args.out}")


def run(args) -> None:
    import unet_convlstm_amd as U
    if not torch.cuda.is_available():
        raise SystemExit("a HIP device is required (this package has no CPU path)")
    if getattr(args, "axes", None):                                   # callers that build their own namespace predate the option
        return run_vector(args, U, torch.device("cuda", 0))
    device = torch.device("cuda", 0)
    print(f"[INFO] Loading checkpoint: {args.checkpoint}")
    model = load_model(U, args.checkpoint, device)
    full_dataset = U.NPZSequenceDataset(args.npz, min_y=None, max_y=None)
    n_train = int(0.8 * len(full_dataset))                           # the split of training, same seed
    n_val = len(full_dataset) - n_train
    generator = torch.Generator().manual_seed(42)
    _, val_ds = torch.utils.data.random_split(full_dataset, [n_train, n_val], generator=generator)
    print(f"[INFO] Dataset loaded. Evaluating on VALIDATION set only ({len(val_ds)} sequences)")
    loader = torch.utils.data.DataLoader(val_ds, batch_size=args.batch, shuffle=False)
    t0 = time.perf_counter()
    loss, mae, rmse, me, report = U.evaluate_report(model, loader, device, full_dataset, use_mask=args.use_mask)
    dt = time.perf_counter() - t0
    if report["n"] <= 0:
        print("[WARNING] No valid pixels found to plot.")
    print("\n" + "=" * 40)
    print(f"Global MAE:        {report['mae']:.4f} m/s")
    print(f"Global RMSE:       {report['rmse']:.4f} m/s")
    print(f"Global Mean Error (Bias): {report['mean_err']:.4f} m/s")
    print(f"Global Error Std:  {report['std_err']:.4f} m/s")
    print("=" * 40)
    print(f"[INFO] loss {loss:.6f}; {len(val_ds)} sequences in {dt:.3f} s; {len(report['scatter_gt'])} points in the balanced sample")
    if args.out:
        np.savez(args.out, loss=np.float64(loss), **flat(report))
        print(f"[INFO] report written to {args.out}")
    if args.plots:
        draw(report, args.plots)


# ---------------------------------------------------------------------------------------------
# --bench
# ---------------------------------------------------------------------------------------------
def _time_alternated(fns: dict, warmup: int, iters: int, spin) -> dict:
    """Median milliseconds per launch of each entry, HIP events around every single launch, the entries alternated.  Every round
    is queued behind a 500 us spin kernel, so the launches wait in the queue and the events see device time, not the host's
    launch cost (these kernels take tens of microseconds)."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(iters):
        spin()
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}


def _numpy_formulas(ds, y, yp, mask):
    """The host flow of get_metrics.py on one batch (statistics only), as the reference computes it."""
    gt, pr = ds.denormalize(y), ds.denormalize(yp)
    if mask is not None:
        v = mask > 0.1
        t = np.nonzero(v)[1]
        gt, pr = gt[v], pr[v]
    else:
        t = np.broadcast_to(np.arange(y.shape[1])[None, :, None, None, None], y.shape).ravel()
        gt, pr = gt.ravel(), pr.ravel()
    d = pr - gt
    out = [np.mean(np.abs(d)), np.sqrt(np.mean(d ** 2)), np.mean(d), np.std(d)]
    out.append([np.mean(np.abs(d[t == k])) for k in range(y.shape[1])])
    out += [np.histogram(gt, 100, (-7.5, 7.5))[0], np.histogram(pr, 100, (-7.5, 7.5))[0], np.histogram(d, 100, (-3, 3))[0]]
    out.append(np.bincount(np.digitize(gt, np.arange(-8.0, 8.05, 0.05)), minlength=322))
    return out


def bench(args) -> None:
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L, ops

    class DS:
        y_transform, y_scale = "asinh", 2.0
        trans_min, trans_max = float(np.arcsinh(-7.5987958908081055 / 2.0)), float(np.arcsinh(8.784920692443848 / 2.0))
        denormalize = U.NPZSequenceDataset.denormalize

    ds = DS()
    dev = torch.device("cuda", 0)
    print(f"# eval_stats against uclstm_metric_sums: median ms per launch over {args.iters} launches each (HIP events, {args.warmup} warm-up "
          f"rounds, entries alternated in one process); GB/s from algorithmic bytes (8 B/pixel, 12 B with a mask)")
    print("# new = uclstm_eval_stats on the model's transposed view (no copy); sums = uclstm_metric_sums on contiguous tensors; "
          "sums+copy = the .contiguous() copy of the view that _Metrics.add makes, then uclstm_metric_sums")
    print(f"{'shape':>20} {'input':>8} {'mask':>5} {'new ms':>9} {'GB/s':>7} {'sums ms':>9} {'GB/s':>7} {'sums+copy ms':>13} {'new/sums':>9} {'new/sums+copy':>14}")
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    stream = ops._stream()
    for shape in ((32, 20, 1, 64, 64), (4, 12, 1, 256, 256)):
        for kind in ("uniform", "skewed"):
            g = torch.Generator().manual_seed(1)
            y = torch.rand(shape, generator=g) * 2 - 1
            if kind == "skewed":
                y[torch.rand(shape, generator=g) < 0.85] = -0.4137
            yp = (y + 0.15 * torch.randn(shape, generator=g)).clamp(-1.2, 1.2)
            mask = (torch.rand(shape, generator=g) > 0.3).float()
            y_d, m_d = y.to(dev), mask.to(dev)
            view = yp.transpose(0, 1).contiguous().to(dev).transpose(0, 1)          # as the model returns it
            yp_c = view.contiguous()
            n = y.numel()
            for use_mask in (False, True):
                rep = U.EvalReport(ds, device=dev)
                m = m_d if use_mask else None
                desc, table = rep._describe(view, y_d, m)                              # as add() builds it: the view is read in place
                assert desc.y_pred == view.data_ptr() and not view.is_contiguous()

                def new():
                    L.check(L.lib.uclstm_eval_stats(desc, stream), "eval_stats")

                def old(p=yp_c):
                    L.check(L.lib.uclstm_metric_sums(ops._p(p), ops._p(y_d), ops._p(m), ops._p(sums), n, ds.y_scale, ds.trans_min,
                                                     ds.trans_max, stream), "metric_sums")

                def old_copy():
                    old(view.contiguous())

                ms = _time_alternated({"new": new, "sums": old, "sums+copy": old_copy}, args.warmup, args.iters,
                                      lambda: L.check(L.lib.uclstm_stream_spin(500, stream), "spin"))
                expect = (args.warmup + args.iters) * int(m.sum().item() if use_mask else n)
                if int(rep._dig.sum().item()) != expect:
                    raise SystemExit("eval_stats counted something else than the pixels it was given")
                gb = n * (12 if use_mask else 8) / 1e6
                print(f"{str(list(shape)):>20} {kind:>8} {str(use_mask):>5} {ms['new']:9.4f} {gb / ms['new']:7.0f} {ms['sums']:9.4f} "
                      f"{gb / ms['sums']:7.0f} {ms['sums+copy']:13.4f} {ms['new'] / ms['sums']:9.2f} {ms['new'] / ms['sums+copy']:14.2f}", flush=True)
    # end to end: evaluate_report against evaluate on one loader, then the host formulas on the same data
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=16, use_skip_lstm=True).to(dev)
    data = U.SyntheticSequences(8, 12, 64, 64, seed=3, device=dev)
    loader = [(data.x, data.y, data.mask)] * 8
    for f in (U.evaluate, U.evaluate_report):
        f(model, loader, dev, ds, True)
    torch.cuda.synchronize()
    res = {}
    for name, f in (("evaluate", U.evaluate), ("evaluate_report", U.evaluate_report)) * 3:
        t0 = time.perf_counter()
        f(model, loader, dev, ds, True)
        torch.cuda.synchronize()
        res.setdefault(name, []).append(time.perf_counter() - t0)
    print(f"# end to end, 8 batches of [8,12,*,64,64], base_ch 16, use_mask: evaluate {1e3 * min(res['evaluate']):.2f} ms, "
          f"evaluate_report {1e3 * min(res['evaluate_report']):.2f} ms (best of 3, result() included)")
    with torch.no_grad():
        out, _ = model(data.x)
        yp_h = torch.stack(list(out), 1).float().cpu().numpy()
    y_h, m_h = data.y.cpu().numpy(), data.mask.cpu().numpy()
    t0 = time.perf_counter()
    for _ in range(8):
        _numpy_formulas(ds, y_h, yp_h, m_h)
    print(f"# for the record: the host numpy formulas (denormalize, 4 global figures, MAE per time step, 3 histograms, digitize) on the same "
          f"8 batches: {1e3 * (time.perf_counter() - t0):.1f} ms (numpy, one host thread)")


def bench_vector(args) -> None:
    """uclstm_eval_stats_vec at Cy = 3 against what it replaces, by the method of bench(): HIP events around every entry, a spin
    kernel in front of every round, the entries alternated, medians; the whole comparison three times over (legs), so that the
    spread between legs says what a difference between entries means."""
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L, ops

    Cy, legs = 3, 3
    ds = object.__new__(U.VectorNPZDataset)                             # the constants only: no file behind it
    ds.Cy, ds.axes, ds.w_channel, ds.h_channel, ds.y_transform = Cy, ("+w", "-h", None), 0, 1, "asinh"
    ds.y_scale = np.array([2.0, 2.0, 0.5])
    ds.min_vel, ds.max_vel = np.array([-7.6, -7.6, -2.0]), np.array([8.8, 8.8, 2.0])
    ds.trans_min, ds.trans_max = np.arcsinh(ds.min_vel / ds.y_scale), np.arcsinh(ds.max_vel / ds.y_scale)

    class One:                                                          # channel c as a scalar dataset
        def __init__(self, c):
            self.y_transform, self.y_scale, self.trans_min, self.trans_max = "asinh", ds.y_scale[c], ds.trans_min[c], ds.trans_max[c]

    dev = torch.device("cuda", 0)
    print(f"# eval_stats_vec at Cy = {Cy}: median ms per entry over {args.iters} rounds (HIP events, {args.warmup} warm-up rounds, entries alternated "
          f"in one process), the median of {legs} legs and their [min .. max]; GB/s of vec from its algorithmic bytes (8 * Cy B/pixel, + 4 with a mask)")
    print("# vec = uclstm_eval_stats_vec with the horizontal pair; vec-nopair = the same launch with w_chan = h_chan = -1 (the per-channel part alone); "
          "3 x scalar = Cy in-place launches of uclstm_eval_stats (the same per-channel statistics); sums_vec = uclstm_metric_sums_vec on contiguous tensors")
    print(f"{'shape':>20} {'input':>8} {'mask':>5} {'vec ms':>24} {'GB/s':>6} {'vec-nopair ms':>24} {'3 x scalar ms':>24} {'sums_vec ms':>24} {'vec/3 x scalar':>15}")
    stream = ops._stream()
    sv = torch.zeros((Cy, 4), dtype=torch.float64, device=dev)
    for shape in ((32, 20, Cy, 64, 64), (4, 12, Cy, 256, 256)):
        B, T, _, H, W = shape
        for kind in ("uniform", "skewed"):
            g = torch.Generator().manual_seed(1)
            y = torch.rand(shape, generator=g) * 2 - 1
            if kind == "skewed":
                y[torch.rand(shape, generator=g) < 0.85] = -0.4137
            yp = (y + 0.15 * torch.randn(shape, generator=g)).clamp(-1.2, 1.2)
            mask = (torch.rand((B, T, 1, H, W), generator=g) > 0.3).float()
            y_d, m_d = y.to(dev), mask.to(dev)
            view = yp.transpose(0, 1).contiguous().to(dev).transpose(0, 1)          # as the model returns it
            yp_c = view.contiguous()
            n_frames, n = B * T, B * T * H * W
            partials = torch.empty((int(L.lib.uclstm_metric_sums_vec_rows(n_frames, Cy, H * W)), Cy, 4), dtype=torch.float64, device=dev)
            for use_mask in (False, True):
                m = m_d if use_mask else None
                rep = U.VectorEvalReport(ds, device=dev)
                desc, _table, _vtable = rep._describe(view, y_d, m)
                assert desc.y_pred == view.data_ptr() and not view.is_contiguous()
                rep_np = U.VectorEvalReport(ds, device=dev)
                desc_np, _t, _v = rep_np._describe(view, y_d, m)
                desc_np.w_chan = desc_np.h_chan = -1
                scalar = []
                for c in range(Cy):
                    r = U.EvalReport(One(c), device=dev)
                    scalar.append((r, r._describe(view[:, :, c:c + 1], y_d[:, :, c:c + 1], m)))
                    assert scalar[-1][1][0].y_pred == view.data_ptr() + 4 * c * H * W

                def vec():
                    L.check(L.lib.uclstm_eval_stats_vec(desc, stream), "eval_stats_vec")

                def vec_nopair():
                    L.check(L.lib.uclstm_eval_stats_vec(desc_np, stream), "eval_stats_vec")

                def three():
                    for _r, (d, _tab) in scalar:
                        L.check(L.lib.uclstm_eval_stats(d, stream), "eval_stats")

                def sums_vec():
                    L.check(L.lib.uclstm_metric_sums_vec(ops._p(yp_c), ops._p(y_d), ops._p(m), ops._p(partials), ops._p(sv), 1, n_frames, Cy, H * W,
                                                         1, ds.target_consts(), stream), "metric_sums_vec")

                fns = {"vec": vec, "vec-nopair": vec_nopair, "3 x scalar": three, "sums_vec": sums_vec}
                runs = [_time_alternated(fns, args.warmup, args.iters, lambda: L.check(L.lib.uclstm_stream_spin(500, stream), "spin"))
                        for _ in range(legs)]
                expect = legs * (args.warmup + args.iters) * int(m.sum().item() if use_mask else n)
                got = [int(v) for v in rep._dig.sum(dim=1).tolist()] + [int(r._dig.sum().item()) for r, _ in scalar]
                if got != [expect] * (2 * Cy) or int(rep._dir.sum().item()) > expect:
                    raise SystemExit(f"the kernels counted something else than the pixels they were given: {got}, expected {expect}")
                ms = {k: sorted(r[k] for r in runs) for k in fns}
                med = {k: v[legs // 2] for k, v in ms.items()}

                def cell(k):
                    return f"{med[k]:8.4f} [{ms[k][0]:.4f} .. {ms[k][-1]:.4f}]"

                gb = n * (8 * Cy + (4 if use_mask else 0)) / 1e6
                print(f"{str(list(shape)):>20} {kind:>8} {str(use_mask):>5} {cell('vec'):>24} {gb / med['vec']:6.0f} {cell('vec-nopair'):>24} "
                      f"{cell('3 x scalar'):>24} {cell('sums_vec'):>24} {med['vec'] / med['3 x scalar']:15.2f}", flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint")
    ap.add_argument("--npz")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--use-mask", action="store_true")
    ap.add_argument("--out", default=None, help="write the report as .npz")
    ap.add_argument("--plots", default=None, metavar="DIR", help="draw the five figures of get_metrics.py into DIR (needs matplotlib)")
    ap.add_argument("--bench", action="store_true", help="time the kernel against uclstm_metric_sums instead of evaluating a checkpoint")
    ap.add_argument("--axes", default=None, metavar="A,B,..", help='vector target: one of +w, -w, +h, -h, none per channel, e.g. "+w,-h,none"')
    ap.add_argument("--tie-horizontal", action="store_true", help="with --axes: the two horizontal channels share one set of constants")
    ap.add_argument("--vector", action="store_true", help="with --bench: time uclstm_eval_stats_vec (profiles/eval_report_vec.txt)")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.bench:
        if args.iters < 50:
            ap.error("--bench needs --iters >= 50")
        (bench_vector if args.vector else bench)(args)
        return
    if not args.checkpoint or not args.npz:
        ap.error("--checkpoint and --npz are required")
    run(args)


if __name__ == "__main__":
    main()
