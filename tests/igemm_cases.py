"""Helpers of tests/test_gpu_igemm_abi.py that need no GPU: the f64 reference of the implicit-GEMM forward family, the case
table and the descriptor builder.  tests/test_cabi_and_host.py pins the reference to PyTorch's own f64 convolutions on the CPU
and checks the dispatch plan of every case with dummy pointers.

The reference restates the contract of include/uclstm.h and nothing else:
  * for output pixel (img, y, x), tap t and source s the source pixel is (y*scale + t/ktap - pad - offY, x*scale + t%ktap - pad -
    offX); it contributes zero outside [0, Hs) x [0, Ws);
  * K order is tap-major over (kseg[0] + kseg[1]), kseg[s] = roundup(C[s], 64);
  * out[pixel][n] = sum_k A[pixel][k] * Wp[n][k];
  * a STORE segment sends columns [n_begin, n_end) to channels [c_off, ...) of its destination at pixel (y*scale + oy,
    x*scale + ox) and drops pixels that fall outside it;
  * K range r of a split-K launch is the (source, 64-channel) chunks [r*cpr, (r+1)*cpr), cpr = ceil(chunks / ksplit), all taps.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops


def roundup(a, b):
    return (a + b - 1) // b * b


# ---------------------------------------------------------------------------------------------
# f64 reference
# ---------------------------------------------------------------------------------------------
def gather_a(n_img, H, W, ktap, scale, pad, srcs):
    """The GEMM's A operand [n_img*H*W][Ktot] in f64.  srcs: [(x [n_img][Hs][Ws][C], offY, offX)]."""
    ksegs = [roundup(x.shape[3], 64) for x, _, _ in srcs]
    kt = sum(ksegs)
    M = n_img * H * W
    A = torch.zeros(M, ktap * ktap * kt, dtype=torch.float64)
    m = torch.arange(M)
    img, y, xx = m // (H * W), (m % (H * W)) // W, m % W
    for t in range(ktap * ktap):
        base = t * kt
        for (x, offY, offX), ks in zip(srcs, ksegs):
            _, Hs, Ws, Cs = x.shape
            ys = y * scale + t // ktap - pad - offY
            xs = xx * scale + t % ktap - pad - offX
            ok = (ys >= 0) & (ys < Hs) & (xs >= 0) & (xs < Ws)
            rows = x.double()[img, ys.clamp(0, Hs - 1), xs.clamp(0, Ws - 1)]
            A[:, base:base + Cs] = torch.where(ok[:, None], rows, torch.zeros_like(rows))
            base += ks
    return A


def gemm_ref(A, wp, kmask=None):
    """(sum_k A*Wp, sum_k |A*Wp|) [M][N] in f64, over the K columns of `kmask` (all when None)."""
    w = wp.double()
    if kmask is not None:
        A, w = A[:, kmask], w[:, kmask]
    return A @ w.t(), A.abs() @ w.abs().t()


def krange_masks(ktap, ksegs, ksplit):
    """Boolean K-column masks of the non-empty K ranges of a split-K launch (header: whole chunks, all taps of a chunk)."""
    kt = sum(ksegs)
    chunks = kt // 64
    cpr = -(-chunks // ksplit)
    chunk_of_col = (torch.arange(ktap * ktap * kt) % kt) // 64
    return [(chunk_of_col >= r * cpr) & (chunk_of_col < (r + 1) * cpr) for r in range(-(-chunks // cpr))]


def scatter_segments(val, n_img, H, W, segs):
    """Destination tensors [n_img][Hd][Wd][C] of the STORE epilogue for GEMM-shaped values val [M][N]: NaN where the contract
    writes nothing.  segs: [(n_begin, n_end, C, c_off, Hd, Wd, scale, oy, ox)]."""
    M = n_img * H * W
    m = torch.arange(M)
    img, y, x = m // (H * W), (m % (H * W)) // W, m % W
    outs = []
    for n0, n1, Cd, c_off, Hd, Wd, sc, oy, ox in segs:
        dst = torch.full((n_img, Hd, Wd, Cd), float("nan"), dtype=torch.float64)
        yd, xd = y * sc + oy, x * sc + ox
        ok = (yd >= 0) & (yd < Hd) & (xd >= 0) & (xd < Wd)
        dst[img[ok], yd[ok], xd[ok], c_off:c_off + n1 - n0] = val[ok][:, n0:n1]
        outs.append(dst)
    return outs


def lstm_rows_to_gates(pre, Hd_p):
    """Panel-row order n = hb*64 + gate*16 + j  ->  [M][4][Hd_p], hidden channel hb*16 + j."""
    M, N = pre.shape
    return pre.view(M, N // 64, 4, 16).permute(0, 2, 1, 3).reshape(M, 4, N // 4)[:, :, :Hd_p]


def lstm_cell_ref(pre, c_prev):
    """train/unet.py:29-35 in f64 on pre-activations [M][4][Hd_p] (i, f, g, o): gates, c_next, h_next."""
    i, f, o = torch.sigmoid(pre[:, 0]), torch.sigmoid(pre[:, 1]), torch.sigmoid(pre[:, 3])
    g = torch.tanh(pre[:, 2])
    c = f * c_prev + i * g
    return torch.stack((i, f, g, o), 1), c, o * torch.tanh(c)


def host_panel(w, cs, ktap, N):
    """f64 panel [N][Ktot] of an OIHW weight [Co][sum(cs)][ktap][ktap] (Co <= N), written from the header's K order; the CPU tests
    use it where the GPU tests read the device panel back."""
    ksegs = [roundup(c, 64) for c in cs]
    kt = sum(ksegs)
    wp = torch.zeros(N, ktap * ktap * kt, dtype=torch.float64)
    for t in range(ktap * ktap):
        base, ch = t * kt, 0
        for c, ks in zip(cs, ksegs):
            wp[:w.shape[0], base:base + c] = w[:, ch:ch + c, t // ktap, t % ktap]
            base, ch = base + ks, ch + c
    return wp


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    shape: int                                   # what uclstm_igemm_fwd_shape must say
    n_img: int
    H: int
    W: int
    srcs: List[Tuple[int, int, int, int, int]]   # (C, Hs, Ws, offY, offX)
    N: int
    ktap: int = 3
    scale: int = 1
    pad: int = 1
    groups: int = 1
    epi: int = L.EPI_STORE
    segs: Optional[list] = None                  # None: one segment, every column, onto the output grid
    bias: bool = True
    affine: bool = False
    relu: bool = False
    stats: bool = False
    pack: str = "conv"                           # conv | convt | lstm | lstm_h
    guard: bool = False                          # S6b: guard rows around every destination
    # split-K
    ksplit: int = 1
    # fused cell
    Hd: int = 0
    opts: Tuple[str, ...] = ()                   # no_c_prev, no_bias, pre_add
    note: str = ""

    @property
    def M(self):
        return self.n_img * self.H * self.W

    @property
    def ksegs(self):
        return [roundup(s[0], 64) for s in self.srcs]

    @property
    def Ktot(self):
        return self.ktap * self.ktap * sum(self.ksegs)

    @property
    def Hd_p(self):
        return roundup(self.Hd, 8)

    def segments(self):
        return self.segs if self.segs is not None else [(0, self.N, self.N, 0, self.H, self.W, 1, 0, 0)]

    def tile_pixels(self):
        return 128 if self.N > 64 else 256


def _convt_segs(Cop, Hd, Wd):
    return [(t * Cop, (t + 1) * Cop, Cop, 0, Hd, Wd, 2, t // 2, t % 2) for t in range(4)]


G = [(24, 9, 11, 0, 0)]                  # the 3 x 9 x 11 grid's plain source: M = 297, one K chunk with a 24-of-64 tail
TWO_PAD = [(24, 9, 11, 0, 0), (16, 6, 9, 1, 1)]        # F.pad left/top 1, right 1, bottom 2
TWO_CROP = [(24, 9, 11, 0, 0), (16, 11, 14, -1, -2)]   # second source larger than the grid: cropped

STORE_CASES = [
    Case("S1", 0, 3, 9, 11, G, 136),
    Case("S2", 1, 3, 9, 11, G, 40),
    Case("S3-k0", 0, 3, 9, 11, TWO_PAD, 136),
    Case("S3-k1", 1, 3, 9, 11, TWO_PAD, 40),
    Case("S3b-k0", 0, 3, 9, 11, TWO_CROP, 136),
    Case("S3b-k1", 1, 3, 9, 11, TWO_CROP, 40),
    Case("S4", 1, 3, 9, 11, [(72, 9, 11, 0, 0)], 16, ktap=1, pad=0, note="N = 16 <= 64 dispatches to the 64x256 shape"),
    Case("S4-k0", 0, 3, 9, 11, [(72, 9, 11, 0, 0)], 136, ktap=1, pad=0, note="the same plain GEMM on the 128x128 shape"),
    Case("S5", 0, 3, 5, 6, [(24, 10, 12, 0, 0)], 136, ktap=2, scale=2, pad=0),
    Case("S5-odd", 0, 3, 5, 6, [(24, 9, 11, 0, 0)], 136, ktap=2, scale=2, pad=0),
    Case("S6", 1, 3, 5, 6, [(24, 5, 6, 0, 0)], 64, ktap=1, pad=0, pack="convt", segs=_convt_segs(16, 11, 13),
         note="N = 64 dispatches to the 64x256 shape"),
    Case("S6-k0", 0, 3, 5, 6, [(24, 5, 6, 0, 0)], 160, ktap=1, pad=0, pack="convt", segs=_convt_segs(40, 11, 13),
         note="N = 4 x 40: the same scatter on the 128x128 shape"),
    Case("S6b", 1, 3, 5, 6, [(24, 5, 6, 0, 0)], 64, ktap=1, pad=0, pack="convt", segs=_convt_segs(16, 9, 11), guard=True),
    Case("S6b-k0", 0, 3, 5, 6, [(24, 5, 6, 0, 0)], 160, ktap=1, pad=0, pack="convt", segs=_convt_segs(40, 9, 11), guard=True),
    Case("S7", 0, 3, 9, 11, G, 136, segs=[(8, 32, 48, 16, 9, 11, 1, 0, 0)], note="N = 136 keeps the case on the 128x128 shape"),
    Case("S8-k0", 0, 3, 9, 11, G, 136, affine=True, relu=True),
    Case("S8-k1", 1, 3, 9, 11, G, 40, affine=True, relu=True),
    Case("S8-k2", 2, 2, 16, 16, [(128, 16, 16, 0, 0)], 136, affine=True, relu=True),
    Case("S9-k0-g3", 0, 3, 9, 11, G, 136, groups=3, stats=True),
    Case("S9-k1-g3", 1, 3, 9, 11, G, 40, groups=3, stats=True),
    Case("S9-k0-g2", 0, 2, 16, 24, [(24, 16, 24, 0, 0)], 136, groups=2, stats=True),
    Case("S9-k1-g2", 1, 2, 16, 24, [(24, 16, 24, 0, 0)], 40, groups=2, stats=True),
    Case("S10-5", 0, 3, 9, 11, [(16, 9, 11, 0, 0)], 24, ktap=5, pad=2),
    Case("S10-7", 0, 3, 9, 11, [(16, 9, 11, 0, 0)], 24, ktap=7, pad=3),
    Case("S10-5-small", 0, 3, 3, 4, [(16, 3, 4, 0, 0)], 24, ktap=5, pad=2),
    Case("S10-7-small", 0, 3, 3, 4, [(16, 3, 4, 0, 0)], 24, ktap=7, pad=3),
    Case("S11-a", 2, 2, 16, 16, [(128, 16, 16, 0, 0)], 136, groups=2, stats=True),
    Case("S11-b", 2, 16, 4, 4, [(64, 4, 4, 0, 0), (64, 4, 4, 0, 0)], 128, stats=True, note="128 pixels per half: groups 1"),
    Case("S11-c", 2, 4, 16, 24, [(128, 16, 24, 0, 0)], 128, groups=2, stats=True),
    Case("S12-a", 2, 1, 4, 128, [(128, 4, 128, 0, 0)], 128, stats=True),
    Case("S12-b", 2, 2, 8, 192, [(64, 8, 192, 0, 0), (64, 8, 192, 0, 0)], 192, groups=2, stats=True),
    Case("S13-a", 3, 1, 4, 64, [(64, 4, 64, 0, 0)], 64, stats=True),
    Case("S13-b", 3, 2, 8, 128, [(64, 8, 128, 0, 0)], 64, groups=2, stats=True),
    Case("S13-c", 3, 5, 4, 64, [(64, 4, 64, 0, 0)], 64, stats=True),
    Case("S13-d", 3, 2, 8, 128, [(64, 8, 128, 0, 0)], 64, stats=True, segs=[(0, 40, 40, 0, 8, 128, 1, 0, 0)]),
    Case("S13-e", 3, 259, 4, 64, [(64, 4, 64, 0, 0)], 64, groups=7, stats=True,
         note="259 tiles on 256 blocks: two tiles per block, the last block one; 37 tiles per group, so three of the six group "
              "boundaries fall inside a block's run"),
]

A01 = [(72, 9, 11, 0, 0), (24, 9, 11, 0, 0)]                    # 128 + 64: three chunks
A2 = [(128, 16, 16, 0, 0), (64, 16, 16, 0, 0)]                  # three chunks on the patch shape
ATOMIC_CASES = (
    [Case(f"A-k0-s{k}", 0, 3, 9, 11, A01, 136, epi=L.EPI_ATOMIC, ksplit=k, bias=False) for k in (1, 2, 8)] +
    [Case(f"A-k1-s{k}", 1, 3, 9, 11, A01, 40, epi=L.EPI_ATOMIC, ksplit=k, bias=False) for k in (1, 2, 8)] +
    [Case(f"A-k2-s{k}", 2, 2, 16, 16, A2, 136, epi=L.EPI_ATOMIC, ksplit=k, bias=False) for k in (1, 2, 8)] +
    [Case("A-k2-s3of5", 2, 2, 16, 16, [(320, 16, 16, 0, 0)], 136, epi=L.EPI_ATOMIC, ksplit=3, bias=False)]
)
ATOMIC_USED = {"s1": 1, "s2": 2, "s8": 3, "s3of5": 3}          # expected uclstm_igemm_ksplit_used


def _lstm(name, shape, n_img, H, W, Cx, Hd, opts=(), single=False):
    Hp = roundup(Hd, 8)
    srcs = [(Hp, H, W, 0, 0)] if single else [(Cx, H, W, 0, 0), (Hp, H, W, 0, 0)]
    return Case(name, shape, n_img, H, W, srcs, 64 * ((Hd + 15) // 16), epi=L.EPI_LSTM, Hd=Hd, opts=tuple(opts),
                pack="lstm_h" if single else "lstm", bias="no_bias" not in opts)


LSTM_CASES = [
    _lstm("L0-hd8", 0, 3, 9, 11, 24, 5, ("pre_add",)),
    _lstm("L0-hd24", 0, 3, 9, 11, 24, 21, ("pre_add",)),
    _lstm("L0-hd64", 0, 3, 9, 11, 24, 64, ("pre_add",)),
    _lstm("L0-no-c-prev", 0, 3, 9, 11, 24, 21, ("no_c_prev",)),
    _lstm("L0-no-bias", 0, 3, 9, 11, 24, 21, ("no_bias",)),
    _lstm("L0-h-only", 0, 3, 9, 11, 24, 21, ("pre_add",), single=True),
    _lstm("L2-tile", 2, 1, 16, 16, 64, 64, ("pre_add",)),
    _lstm("L2-strip", 2, 1, 4, 128, 64, 64, ("pre_add",)),
    _lstm("L2-no-c-prev-no-bias", 2, 1, 16, 16, 64, 64, ("no_c_prev", "no_bias")),
    _lstm("L2-h-only", 2, 1, 16, 16, 64, 128, ("pre_add",), single=True),
]

# uclstm_igemm_fwd_group: three unlike members, and four members
GROUP_A = [_lstm("G-lstm16", 2, 1, 16, 16, 64, 64, ("pre_add",)),
           Case("G-slab", 2, 4, 8, 8, [(128, 8, 8, 0, 0), (64, 8, 8, 0, 0)], 136, epi=L.EPI_ATOMIC, ksplit=2, bias=False),
           _lstm("G-lstm-strip", 2, 1, 4, 128, 64, 64)]
GROUP_B = GROUP_A + [Case("G-slab1", 2, 2, 16, 16, A2, 136, epi=L.EPI_ATOMIC, ksplit=8, bias=False)]

ALL_CASES = STORE_CASES + ATOMIC_CASES + LSTM_CASES


# ---------------------------------------------------------------------------------------------
# descriptor
# ---------------------------------------------------------------------------------------------
DUMMY = 1 << 20


def pack_desc(c: Case) -> L.PackDesc:
    """Pack descriptor of the case's weight tensor (weight_shape): its last three output channels and the last three input channels
    of a second source are padding, so the panel carries the zero rows and columns a real layer has."""
    if c.pack == "convt":
        return ops.convt_pack_desc(c.srcs[0][0], c.N // 4 - 3)
    if c.pack == "lstm":
        return ops.lstm_pack_desc(c.Hd, c.srcs[0][0], c.ktap)
    if c.pack == "lstm_h":
        return ops.lstm_half_pack_desc(c.Hd, 24, "h", c.ktap)
    taps = c.ktap * c.ktap
    cv = conv_valid(c)
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = c.N, taps, len(c.srcs)
    for i in range(len(c.srcs)):
        d.kseg[i], d.cvalid[i] = c.ksegs[i], cv[i]
    d.choff[0], d.choff[1] = 0, cv[0]
    d.Ktot = c.Ktot
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, c.N - 3, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = sum(cv) * taps, taps, 1, 0
    return d


def conv_valid(c: Case):
    return [s[0] if i == 0 else s[0] - 3 for i, s in enumerate(c.srcs)]


def weight_shape(c: Case):
    if c.pack == "convt":
        return (c.srcs[0][0], c.N // 4 - 3, 2, 2)
    if c.pack == "lstm":
        return (4 * c.Hd, c.srcs[0][0] + c.Hd, c.ktap, c.ktap)
    if c.pack == "lstm_h":
        return (4 * c.Hd, 24 + c.Hd, c.ktap, c.ktap)
    return (c.N - 3, sum(conv_valid(c)), c.ktap, c.ktap)


def build_desc(c: Case, src_ptrs=None, wp=DUMMY, seg_ptrs=None, bias=None, col_scale=None, col_shift=None, stats=None, c_prev=None,
               c_out=None, h_out=None, gates_out=None, pre_add=None, acc_out=None, acc_ld=0, acc_slab=0) -> L.IgemmDesc:
    """uclstm_igemm_desc of a case from raw addresses (integers or None)."""
    d = L.IgemmDesc()
    d.n_img, d.H, d.W, d.groups = c.n_img, c.H, c.W, c.groups
    d.ktap, d.scale, d.pad, d.nsrc = c.ktap, c.scale, c.pad, len(c.srcs)
    for i, (Cs, Hs, Ws, offY, offX) in enumerate(c.srcs):
        s = d.src[i]
        s.ptr = src_ptrs[i] if src_ptrs else DUMMY
        s.C, s.Hs, s.Ws, s.offY, s.offX = Cs, Hs, Ws, offY, offX
    d.wp, d.N, d.Ktot = wp, c.N, c.Ktot
    d.bias, d.col_scale, d.col_shift = bias, col_scale, col_shift
    d.relu, d.epi = int(c.relu), c.epi
    if c.epi == L.EPI_STORE:
        segs = c.segments()
        d.nseg = len(segs)
        for i, (n0, n1, Cd, c_off, Hd, Wd, sc, oy, ox) in enumerate(segs):
            g = d.seg[i]
            g.ptr = seg_ptrs[i] if seg_ptrs else DUMMY
            g.n_begin, g.n_end, g.C, g.c_off, g.Hd, g.Wd, g.scale, g.oy, g.ox = n0, n1, Cd, c_off, Hd, Wd, sc, oy, ox
        d.stats = stats
    elif c.epi == L.EPI_LSTM:
        d.Hd_p = c.Hd_p
        d.c_prev, d.c_out, d.h_out, d.gates_out, d.pre_add = c_prev, c_out, h_out, gates_out, pre_add
    else:
        d.acc_out, d.acc_ld, d.ksplit, d.acc_slab = acc_out, acc_ld, c.ksplit, acc_slab
    return d


def dummy_desc(c: Case) -> L.IgemmDesc:
    """The case's descriptor with aligned dummy pointers: enough for the validation-only entry points."""
    if c.epi == L.EPI_LSTM:
        return build_desc(c, c_out=DUMMY, h_out=DUMMY, c_prev=DUMMY, gates_out=DUMMY, bias=DUMMY)
    if c.epi == L.EPI_ATOMIC:
        return build_desc(c, acc_out=DUMMY, acc_ld=c.N + 8, acc_slab=c.M * (c.N + 8))
    return build_desc(c, bias=DUMMY, stats=DUMMY if c.stats else None)


def stats_tiles(c: Case):
    """Pixel indices of every `stats` slot, in slot order [groups * tiles_per_group].  A tile is a run of 128 (N > 64) or 256
    consecutive pixels of its group.  On images wider than 64 pixels the patch and ring kernels cut an image into 4-row x
    64-column strip tiles instead (the same number of tiles, none crossing an image, so none crosses a group): the patch kernel
    numbers them (image, band, strip) and fills two slots per tile, rows 0-1 and rows 2-3 of the band; the ring kernel numbers
    them (image, strip, band)."""
    tp = c.tile_pixels()
    mg = c.M // c.groups
    tpg = -(-mg // tp)
    if c.shape in (2, 3) and c.W > 64:
        yy, xx = torch.meshgrid(torch.arange(4), torch.arange(64), indexing="ij")
        tiles, bands, strips = [], c.H // 4, c.W // 64
        for img in range(c.n_img):
            order = [(b, s) for b in range(bands) for s in range(strips)] if c.shape == 2 else \
                    [(b, s) for s in range(strips) for b in range(bands)]
            for b, s in order:
                pix = ((img * c.H + 4 * b + yy) * c.W + 64 * s + xx)
                tiles += [pix[:2].reshape(-1), pix[2:].reshape(-1)] if c.shape == 2 else [pix.reshape(-1)]
    else:
        tiles = [torch.arange(g * mg + t * tp, g * mg + min(mg, (t + 1) * tp)) for g in range(c.groups) for t in range(tpg)]
    assert len(tiles) == c.groups * tpg
    assert all(int(p.min()) // mg == i // tpg == int(p.max()) // mg for i, p in enumerate(tiles))
    assert torch.equal(torch.cat(tiles).sort().values, torch.arange(c.M))
    return tiles


def stats_runs(c: Case):
    """[(slots that must hold zeros, slot that holds the sum, pixel indices of the sum)] over all `stats` slots.  Every kernel but
    the ring kernel fills each slot with its own tile.  The ring kernel runs min(tiles, 256) persistent blocks of ceil(tiles /
    blocks) consecutive tiles; a block adds up its consecutive tiles of ONE group in registers, writes the sum into the last
    slot of that run and zeros into the others (the consumer adds all slots of a group)."""
    tiles = stats_tiles(c)
    if c.shape != 3:
        return [([], i, p) for i, p in enumerate(tiles)]
    n = len(tiles)
    tpg = n // c.groups
    per = -(-n // min(n, 256))
    runs = []
    for b0 in range(0, n, per):
        run = []
        for t in range(b0, min(n, b0 + per)):
            run.append(t)
            if t + 1 == min(n, b0 + per) or (t + 1) // tpg != t // tpg:
                runs.append((run[:-1], run[-1], torch.cat([tiles[k] for k in run])))
                run = []
    assert sorted(z for r in runs for z in r[0] + [r[1]]) == list(range(n))
    return runs


def group_blocks_expected(cases):
    """Sum of the members' own grids, each rounded up to a multiple of 8 (header: uclstm_igemm_fwd_group)."""
    total = 0
    for c in cases:
        tiles = c.M // 256 * (-(-c.N // 128))
        if c.epi == L.EPI_ATOMIC:
            tiles *= int(L.lib.uclstm_igemm_ksplit_used(c.Ktot, c.ktap, c.ksplit))
        total += roundup(tiles, 8)
    return total
