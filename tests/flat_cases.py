"""Cases of the flat forward kernel (csrc/igemm_fwd.hip, igemm_fwd_flat_kernel: uclstm_igemm_fwd_shape == 4), its near misses,
and the runner that tests/test_gpu_igemm_flat.py uses in its own process and in a child with UCLSTM_FWD_FLAT=0.

The kernel takes STORE descriptors whose A operand is a plain row gather: ktap 1 on the output grid (ConvTranspose2d forward)
and ktap 2 / scale 2 on a source twice the grid (its input gradient), one source with C % 64 == 0 or C < 64, K <= 512, 256 | pixels per
group.  Shapes are the smallest that reach each mechanism:
  * one tile, one K-step, four scattered segments (F-convt);
  * 2 and 5 K-steps, so the three-slot ring wraps off its own period (F-k2, F-k5);
  * N = 192: zero panel rows in the second row tile, plain and with c_off into a wider destination (F-n192, F-n192-coff);
  * the 2x2 gather (F-tap2);
  * affine + ReLU + bias (F-affine);
  * statistics rows over two groups, with zero panel rows (F-stats);
  * more tiles than blocks: 259 tiles on 256 persistent blocks, so three blocks run two tiles and the ring, the cursor of the
    loads and the statistics exchange cross a tile boundary -- with one K-step per tile (F-259, the reasoning of case S13-e) and
    with four (F-259-tap2).
  * N = 64 with statistics over two groups (F-n64): the panel-row waves 4 .. 7 of the block only stage, and a tile fills ONE
    statistics row of 256 pixels (the layout of the 64 x 256 per-tap shape it replaces; its bit-identity partner is that shape);
  * the same with a source of 24 channels (F-c24, the pre-gathered first layer: 48-byte pixel rows, five of the eight 16-byte
    pieces of every staged row are zero fill).
"""
from igemm_cases import Case, _convt_segs

FLAT_CASES = [
    Case("F-convt", 4, 2, 8, 16, [(64, 8, 16, 0, 0)], 256, ktap=1, pad=0, pack="convt", segs=_convt_segs(64, 16, 32)),
    Case("F-k2", 4, 2, 8, 16, [(128, 8, 16, 0, 0)], 128, ktap=1, pad=0),
    Case("F-k5", 4, 2, 8, 16, [(320, 8, 16, 0, 0)], 128, ktap=1, pad=0),
    Case("F-n192", 4, 2, 8, 16, [(128, 8, 16, 0, 0)], 192, ktap=1, pad=0),
    Case("F-n192-coff", 4, 2, 8, 16, [(128, 8, 16, 0, 0)], 192, ktap=1, pad=0, segs=[(0, 192, 256, 32, 8, 16, 1, 0, 0)]),
    Case("F-tap2", 4, 2, 8, 16, [(64, 16, 32, 0, 0)], 128, ktap=2, scale=2, pad=0),
    Case("F-affine", 4, 2, 8, 16, [(128, 8, 16, 0, 0)], 128, ktap=1, pad=0, affine=True, relu=True),
    Case("F-stats", 4, 4, 8, 16, [(128, 8, 16, 0, 0)], 192, ktap=1, pad=0, groups=2, stats=True),
    Case("F-n64", 4, 4, 8, 16, [(64, 8, 16, 0, 0)], 64, ktap=1, pad=0, groups=2, stats=True),
    Case("F-c24", 4, 4, 8, 16, [(24, 8, 16, 0, 0)], 64, ktap=1, pad=0, groups=2, stats=True),
    Case("F-259", 4, 259, 4, 64, [(64, 4, 64, 0, 0)], 128, ktap=1, pad=0, groups=7, stats=True),
    Case("F-259-tap2", 4, 259, 4, 64, [(64, 8, 128, 0, 0)], 128, ktap=2, scale=2, pad=0, groups=7, stats=True),
]

# (case, why it misses): each takes the kernel it took before the flat kernel existed -- a per-tap shape
NEAR_MISSES = [
    (Case("M-c72", 0, 2, 8, 16, [(72, 8, 16, 0, 0)], 128, ktap=1, pad=0), "C % 64 != 0"),
    (Case("M-297", 0, 3, 9, 11, [(64, 9, 11, 0, 0)], 128, ktap=1, pad=0), "297 pixels: not a multiple of 256"),
    (Case("M-odd-src", 0, 2, 8, 16, [(64, 15, 32, 0, 0)], 128, ktap=2, scale=2, pad=0), "Hs = 2H - 1"),
    (Case("M-two-src", 0, 2, 8, 16, [(64, 8, 16, 0, 0), (64, 8, 16, 0, 0)], 128, ktap=1, pad=0), "a second source"),
    (Case("M-offset", 0, 2, 8, 16, [(64, 8, 16, 1, 0)], 128, ktap=1, pad=0), "a non-zero offset"),
    (Case("M-tap1-scale2", 0, 2, 8, 16, [(64, 16, 32, 0, 0)], 128, ktap=1, scale=2, pad=0), "ktap 1 with scale 2"),
    (Case("M-tap3", 0, 2, 8, 16, [(64, 8, 16, 0, 0)], 128, ktap=3, pad=1), "ktap 3 (one chunk: not the patch loop either)"),
    (Case("M-k1024", 0, 2, 8, 16, [(1024, 8, 16, 0, 0)], 128, ktap=1, pad=0), "K > 512: the per-tap loop's main loop carries the launch"),
    (Case("M-k1024-tap2", 0, 2, 8, 16, [(256, 16, 32, 0, 0)], 128, ktap=2, scale=2, pad=0), "K = 4 x 256 > 512"),
    (Case("M-n64-c72", 1, 2, 8, 16, [(72, 8, 16, 0, 0)], 64, ktap=1, pad=0), "N = 64 with C % 64 != 0: the 64 x 256 shape"),
]

REPEATS = 8


def run_all(dtype_name, path):
    """Launch every flat case through the C ABI on seeded operands (REPEATS times each, one process) and save the raw bytes of every
    destination and the statistics to `path`: {case: {"shape", "out": [repeat][segment] int16, "stats": [repeat] f32}}.  The
    operands depend on the case name and the dtype only, so two processes see the same bits."""
    import ctypes as C

    import torch

    import igemm_cases as IC
    from unet_convlstm_amd import ops
    L = IC.L
    dtype = getattr(torch, dtype_name)
    res = {}
    for c in FLAT_CASES:
        xd, wp, _, keep = operands(c, dtype)
        segs = c.segments()
        tiles = IC.stats_tiles(c) if c.stats else None
        rec = {"out": [], "stats": []}
        for _ in range(REPEATS):
            outs = [torch.full((c.n_img, s[4], s[5], s[2]), 0x7FE5, dtype=torch.int16, device="cuda") for s in segs]
            stats = torch.full((len(tiles), c.N, 2), float("nan"), device="cuda") if c.stats else None
            d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), [o.data_ptr() for o in outs],
                              *[None if t is None else t.data_ptr() for t in keep], stats.data_ptr() if c.stats else None)
            rec["shape"] = int(L.lib.uclstm_igemm_fwd_shape(C.byref(d)))
            L.check(L.kernels(dtype).uclstm_igemm_fwd(C.byref(d), ops._stream()), c.name)
            torch.cuda.synchronize()
            rec["out"].append([o.cpu() for o in outs])
            rec["stats"].append(stats.cpu() if c.stats else None)
        res[c.name] = rec
    torch.save(res, path)


def operands(c, dtype):
    """Device activations and panel, the host copies, and the epilogue vectors (bias, col_scale, col_shift) of a case."""
    import torch

    import igemm_cases as IC
    from unet_convlstm_amd import ops
    torch.manual_seed(4000 + sum(map(ord, c.name)))
    xs = [(torch.randn(c.n_img, Hs, Ws, Cs) * 0.8).to(dtype) for Cs, Hs, Ws, _, _ in c.srcs]
    xd = [x.cuda().contiguous() for x in xs]
    fan = c.ktap * c.ktap * sum(s[0] for s in c.srcs)
    w = (torch.randn(IC.weight_shape(c)) * (1.6 / fan ** 0.5)).cuda()
    wp = ops.pack_weights(IC.pack_desc(c), w, dtype=dtype)
    assert tuple(wp.shape) == (c.N, c.Ktot)
    bias = torch.randn(c.N) * 0.5 if c.bias else None
    col_scale = (torch.rand(c.N) + 0.5) * torch.where(torch.arange(c.N) % 3 == 0, -1.0, 1.0) if c.affine else None
    col_shift = torch.randn(c.N) * 0.5 if c.affine else None
    host = (xs, bias, col_scale, col_shift)
    keep = [None if t is None else t.float().cuda().contiguous() for t in (bias, col_scale, col_shift)]
    return xd, wp, host, keep
