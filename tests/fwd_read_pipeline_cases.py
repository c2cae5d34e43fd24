"""The launches of tests/test_gpu_fwd_read_pipeline.py, run as a script in a process of its own (the kernel switches
UCLSTM_FWD_C64 / UCLSTM_FWD_PATCH are read once per process):

    python tests/fwd_read_pipeline_cases.py OUT.pt bfloat16|float16 ring|patch REF

Every case is launched through `ops`, its outputs go to OUT.pt, and with REF = 1 each output is also compared here, on the device,
with an f64 reference built from the same 16-bit operands (nine shifted f64 matrix products per source).  The bounds are those of
tests/test_gpu_igemm_abi.py: 16-bit outputs max(u16 * 1.01 * |ref|, floor) + 2^-21 * mag, f32 outputs c * mag with
c = max(2e-6, (Ktot / 32 + ksplit + 2) * 2^-24), the fused cell as stated there.  Saved per output: the worst |err| / bound.
"""
import os
import sys

import torch
import torch.nn.functional as F

if __name__ == "__main__":          # the test module imports this file for its case tables only
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

E_ACT = 2.0 ** -21

#             name           imgs H    W   sources     Co  groups  shape the patch arm must take
RING_CASES = [("three_tiles", 3, 172, 256, [64], 64, 3),        # 516 tiles on 256 blocks: three per block, an image boundary inside a run
              ("one_tile_per_image", 5, 4, 64, [64], 64, 5),    # every tile crosses an image boundary
              ("tall_single_image", 1, 8, 64, [64], 64, 1)]
STORE_CASES = [("single_chunk", 8, 16, 16, [64], 128, 2, 0),    # K = 576: the router keeps one-chunk STORE launches on the per-tap loop
               ("three_chunks", 4, 16, 16, [192], 128, 2, 2),   # odd chunk count: the patch buffers alternate
               ("two_sources", 4, 16, 16, [64, 64], 128, 1, 2),  # the source switches at the chunk boundary
               ("partial_last_tile", 5, 12, 12, [128], 128, 1, 0),   # M = 720: the patch shape needs 256 | M, both arms run the per-tap loop
               ("partial_panel_tile", 4, 16, 16, [128], 192, 1, 2)]  # N = 192: the second 128-row tile is half empty
SLAB_CASE = ("slabs", 4, 16, 16, [128], 128, 2)                 # split-K, one chunk per range: `more` is false from the first tap


def u16(dt):
    return 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11


def conv_ref(xs, w, bias, chans=None):
    """(ref, mag) [pixels, Co] f64 of the 3x3 / pad 1 convolution of the NHWC sources with the OIHW weight (`chans`: only these
    input channels, a split-K range)."""
    N, H, W, _ = xs[0].shape
    Co = w.shape[0]
    ref = torch.zeros(N * H * W, Co, dtype=torch.float64, device="cuda")
    mag = torch.zeros_like(ref)
    wd = w.double()
    c0 = 0
    for x in xs:
        C = x.shape[3]
        xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
        lo, hi = (0, C) if chans is None else (max(chans[0] - c0, 0), min(chans[1] - c0, C))
        if lo < hi:
            for dy in range(3):
                for dx in range(3):
                    a = xp[:, dy:dy + H, dx:dx + W, lo:hi].reshape(-1, hi - lo)
                    wt = wd[:, c0 + lo:c0 + hi, dy, dx].t().contiguous()
                    ref += a @ wt
                    mag += a.abs() @ wt.abs()
        c0 += C
    if bias is not None:
        ref += bias.double()
        mag += bias.double().abs()
    return ref, mag


def worst_16bit(got, ref, term, dt):
    floor = 2.0 ** -25 if dt == torch.float16 else 0.0
    bound = (u16(dt) * 1.01 * ref.abs()).clamp(min=floor) + term + 1e-30
    return float(((got.double().reshape(ref.shape) - ref).abs() / bound).max())


def worst_f32(got, ref, bound):
    return float(((got.double().reshape(ref.shape) - ref).abs() / (bound + 1e-30)).max())


def rnd(dt, *shape, scale=0.7):
    return (torch.randn(*shape) * scale).to(dt).cuda()


def store_case(res, dt, want_ref, name, N, H, W, cs, Co, groups):
    xs = [rnd(dt, N, H, W, c) for c in cs]
    w = (torch.randn(Co, sum(cs), 3, 3) * 0.05).to(dt).float().cuda()      # representable: the panel holds exactly these values
    b = (torch.randn(Co) * 0.3).cuda()
    pd = ops.conv_pack_desc(Co, sum(cs), cs, cs)
    wp, bp = ops.pack_weights(pd, w, dtype=dt), ops.pack_bias(pd, b)
    out = torch.full((N, H, W, Co), float("nan"), dtype=dt, device="cuda")
    tpg = U._lib.lib.uclstm_igemm_tiles_per_group(N, H, W, groups, Co)
    stats = torch.full((groups, tpg, Co, 2), float("nan"), device="cuda")
    n0 = len(ops.SHAPE_LOG)
    ops.igemm_store([ops.SrcView(t) for t in xs], wp, (H, W), N, [(out, 0, Co, 0, 1, 0, 0)], ktap=3, pad=1, groups=groups, bias=bp, stats=stats)
    res[name] = {"out": out.cpu(), "stats": stats.sum(1).cpu(), "shapes": ops.SHAPE_LOG[n0:]}
    if want_ref:
        ref, mag = conv_ref(xs, w, b)
        res[name]["worst"] = {"out": worst_16bit(out, ref, 2.0 ** -21 * mag, dt)}
        # statistics: the f64 sums of the kernel's OWN stored values, at 2e-6 of sum |terms|.  That is the per-slot bound of the ABI
        # test; here the slots of a group are added in f64, and the sum of the slots' errors is within the sum of their bounds.
        q = out.double().reshape(groups, -1, Co)
        s = torch.stack((q.sum(1), (q * q).sum(1)), -1)
        sm = torch.stack((q.abs().sum(1), (q * q).sum(1)), -1)
        res[name]["worst"]["stats"] = worst_f32(stats.double().sum(1), s, 2e-6 * sm)


def slab_case(res, dt, want_ref, name, N, H, W, cs, Co, ks):
    xs = [rnd(dt, N, H, W, c) for c in cs]
    w = (torch.randn(Co, sum(cs), 3, 3) * 0.05).to(dt).float().cuda()
    pd = ops.conv_pack_desc(Co, sum(cs), cs, cs)
    wp = ops.pack_weights(pd, w, dtype=dt)
    nsl = ops.ksplit_used(wp.shape[1], ks)
    assert nsl == ks == sum(cs) // 64, "one 64-channel chunk per K range"
    acc = torch.full((nsl, N * H * W, wp.shape[0]), float("nan"), device="cuda")
    n0 = len(ops.SHAPE_LOG)
    ops.igemm_atomic([ops.SrcView(t) for t in xs], wp, (H, W), N, acc, ks, ktap=3, pad=1, slabs=True)
    res[name] = {"acc": acc.cpu(), "shapes": ops.SHAPE_LOG[n0:]}
    if want_ref:
        coeff = max(2e-6, (wp.shape[1] / 32 + ks + 2) * 2.0 ** -24)
        worst = 0.0
        for r in range(nsl):
            ref, mag = conv_ref(xs, w, None, chans=(64 * r, 64 * r + 64))
            worst = max(worst, worst_f32(acc[r, :, :Co], ref, coeff * mag))
        res[name]["worst"] = {"acc": worst}


def lstm_operands(dt, B, H, W, Cx, Hd):
    x, h = rnd(dt, B, H, W, Cx, scale=0.5), rnd(dt, B, H, W, Hd, scale=0.5)
    c = torch.randn(B, H, W, Hd).cuda()
    w = (torch.randn(4 * Hd, Cx + Hd, 3, 3) * 0.05).to(dt).float().cuda()
    bias = (torch.randn(4 * Hd) * 0.2).cuda()
    pd = ops.lstm_pack_desc(Hd, Cx)
    wp, bp = ops.pack_weights(pd, w, dtype=dt), ops.pack_bias(pd, bias)
    outs = (torch.full_like(c, float("nan")), torch.full_like(h, float("nan")),
            torch.full((B, H, W, 4 * Hd), float("nan"), dtype=dt, device="cuda"))
    return x, h, c, w, bias, wp, bp, outs


def lstm_worst(dt, x, h, c, w, bias, wp, outs):
    """tests/test_gpu_igemm_abi.py, fused cell: the gate blocks of the OIHW weight are i, f, g, o."""
    Hd = h.shape[3]
    c_out, h_out, gates = outs
    pre, mag = conv_ref([x, h], w, bias)
    pre, mag = pre.view(-1, 4, Hd), mag.view(-1, 4, Hd)
    cp = c.double().view(-1, Hd)
    i, f, o = torch.sigmoid(pre[:, 0]), torch.sigmoid(pre[:, 1]), torch.sigmoid(pre[:, 3])
    g = torch.tanh(pre[:, 2])
    cref = f * cp + i * g
    href = o * torch.tanh(cref)
    gref = torch.stack((i, f, g, o), 1)
    dpre = max(2e-6, (wp.shape[1] / 32 + 1 + 2) * 2.0 ** -24) * mag
    dg = torch.stack((dpre[:, 0] / 4, dpre[:, 1] / 4, dpre[:, 2], dpre[:, 3] / 4), 1) + E_ACT
    dc = cp.abs() * dg[:, 1] + g.abs() * dg[:, 0] + i.abs() * dg[:, 2] + E_ACT
    return {"c": worst_f32(c_out, cref, dc), "h": worst_16bit(h_out, href, dg[:, 3] + dc + E_ACT, dt),
            "gates": worst_16bit(gates.view(-1, 4, Hd), gref, dg, dt)}


def lstm_case(res, dt, want_ref, name, B, H, W, Cx, Hd):
    x, h, c, w, bias, wp, bp, outs = lstm_operands(dt, B, H, W, Cx, Hd)
    n0 = len(ops.SHAPE_LOG)
    ops.igemm_lstm(x, h, wp, bp, c, *outs)
    res[name] = {"c": outs[0].cpu(), "h": outs[1].cpu(), "gates": outs[2].cpu(), "shapes": ops.SHAPE_LOG[n0:]}
    if want_ref:
        res[name]["worst"] = lstm_worst(dt, x, h, c, w, bias, wp, outs)


def group_case(res, dt, want_ref, name, patch_on):
    """Two independent cells (one image per tile, four images per tile) as ONE group launch; with the patch loop switched off the
    group entry point does not exist for them and each member is launched on its own."""
    members = [lstm_operands(dt, 2, 16, 16, 64, 64), lstm_operands(dt, 8, 8, 8, 64, 64)]
    items = [ops._lstm_desc(x, h, wp, bp, c, *outs) for x, h, c, w, bias, wp, bp, outs in members]
    n0 = len(ops.SHAPE_LOG)
    K = ops._k(members[0][5])
    if patch_on:
        assert ops.group_launchable([it[0] for it in items])
        ops.igemm_group(items, K)
    else:
        for it in items:
            ops._igemm_launch(it, K, "igemm_fwd_lstm", "igemm_fwd(lstm)")
    res[name] = {"shapes": ops.SHAPE_LOG[n0:]}
    worst = {}
    for m, (x, h, c, w, bias, wp, bp, outs) in enumerate(members):
        res[name].update({f"c{m}": outs[0].cpu(), f"h{m}": outs[1].cpu(), f"gates{m}": outs[2].cpu()})
        if want_ref:
            worst.update({f"{k}{m}": v for k, v in lstm_worst(dt, x, h, c, w, bias, wp, outs).items()})
    if want_ref:
        res[name]["worst"] = worst


def main():
    out_file, dt, family, want_ref = sys.argv[1], getattr(torch, sys.argv[2]), sys.argv[3], sys.argv[4] == "1"
    res = {}
    with ops.compute_dtype(dt):
        torch.manual_seed(77)
        ops.SHAPE_LOG = []
        if family == "ring":
            for name, N, H, W, cs, Co, groups in RING_CASES:
                store_case(res, dt, want_ref, name, N, H, W, cs, Co, groups)
        else:
            for name, N, H, W, cs, Co, groups, _ in STORE_CASES:
                store_case(res, dt, want_ref, name, N, H, W, cs, Co, groups)
            slab_case(res, dt, want_ref, *SLAB_CASE)
            lstm_case(res, dt, want_ref, "lstm_4x4", 32, 4, 4, 64, 64)          # sixteen images per tile
            group_case(res, dt, want_ref, "group_of_two", os.environ.get("UCLSTM_FWD_PATCH") != "0")
        torch.cuda.synchronize()
    torch.save(res, out_file)


if __name__ == "__main__":
    main()
