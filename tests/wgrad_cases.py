"""Helpers of tests/test_gpu_wgrad_abi.py that need no GPU: the f64 reference of the weight-gradient GEMM family, the case table
and the descriptor builder.  tests/test_cabi_and_host.py pins the reference to PyTorch's own f64 autograd on the CPU and checks
the dispatch plan of every case with dummy pointers.

The reference restates the contract of include/uclstm.h and nothing else:
  * dWp[n][k] = sum over output pixels of dY[pixel][n] * A[pixel][k], A as in the forward family (igemm_cases.gather_a);
  * column n in [n_begin, n_end) of segment i reads seg.ptr[img][y*scale + oy][x*scale + ox][c_off + n - n_begin], zero when that
    pixel lies outside Hd x Wd; a column that no segment covers is zero;
  * slab mode stores `splits` partial panels whose sum is dWp, atomic mode adds dWp to what the panel holds.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

import igemm_cases as IC
from igemm_cases import TWO_CROP, TWO_PAD, roundup
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops


# ---------------------------------------------------------------------------------------------
# f64 reference
# ---------------------------------------------------------------------------------------------
def gather_dy(n_img, H, W, N, segs):
    """The GEMM's dY operand [n_img*H*W][N] in f64.  segs: [(t [n_img][Hd][Wd][C], n_begin, n_end, c_off, scale, oy, ox)]."""
    M = n_img * H * W
    dY = torch.zeros(M, N, dtype=torch.float64)
    m = torch.arange(M)
    img, y, x = m // (H * W), (m % (H * W)) // W, m % W
    for t, n0, n1, c_off, sc, oy, ox in segs:
        _, Hd, Wd, _ = t.shape
        yd, xd = y * sc + oy, x * sc + ox
        ok = (yd >= 0) & (yd < Hd) & (xd >= 0) & (xd < Wd)
        rows = t[img, yd.clamp(0, Hd - 1), xd.clamp(0, Wd - 1), c_off:c_off + n1 - n0].double()
        dY[:, n0:n1] = torch.where(ok[:, None], rows, torch.zeros_like(rows))
    return dY


def wgrad_ref(n_img, H, W, N, ktap, scale, pad, srcs, segs):
    """(dWp, mag) [N][Ktot] in f64: dWp = dY^T A and mag = |dY|^T |A|.  srcs as gather_a, segs as gather_dy."""
    dY = gather_dy(n_img, H, W, N, segs)
    A = IC.gather_a(n_img, H, W, ktap, scale, pad, srcs)
    ref = dY.t() @ A
    return ref, dY.abs_().t() @ A.abs_()


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
@dataclass
class WCase:
    name: str
    shape: int                                   # what uclstm_igemm_wgrad_shape must say
    n_img: int
    H: int
    W: int
    srcs: List[Tuple[int, int, int, int, int]]   # (C, Hs, Ws, offY, offX)
    N: int
    ktap: int = 3
    scale: int = 1
    pad: int = 1
    dys: Optional[list] = None                   # dY tensors (C, Hd, Wd); None: one dense [n_img][H][W][N]
    segs: Optional[list] = None                  # (n_begin, n_end, index into dys, c_off, scale, oy, ox); None: every column of dys[0]
    kind: str = "conv"                           # conv | convt: which PyTorch operation the CPU test differentiates
    atomic_shape: int = -1                       # kernel 4 only: where the same descriptor goes with slab = 0
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

    def dy_tensors(self):
        return self.dys if self.dys is not None else [(self.N, self.H, self.W)]

    def segments(self):
        return self.segs if self.segs is not None else [(0, self.N, 0, 0, 1, 0, 0)]


def _on_grid(H, W, *cs):
    return [(c, H, W, 0, 0) for c in cs]


def _convt(name, Cop, note=""):
    """ConvTranspose2d(k2, s2) weight gradient: a 1x1 GEMM over the 5 x 6 input grid whose row block t = (ty, tx) reads the
    10 x 12 output gradient at (2y + ty, 2x + tx)."""
    return WCase(name, 0, 3, 5, 6, [(24, 5, 6, 0, 0)], 4 * Cop, ktap=1, pad=0, dys=[(Cop, 10, 12)], kind="convt",
                 segs=[(t * Cop, (t + 1) * Cop, 0, 0, 2, t // 2, t % 2) for t in range(4)], note=note)


def _lstm(name, shape, n_img, H, W, Cx, Hd):
    """Gate-convolution gradient: sources x and h, dY the [pixels][4*Hd_p] gate tensor; N and Ktot of the model's own descriptor."""
    ud = ops.lstm_wgrad_unpack_desc(Hd, Cx, 3)
    c = WCase(name, shape, n_img, H, W, _on_grid(H, W, roundup(Cx, 8), roundup(Hd, 8)), ud.N)
    assert c.Ktot == ud.Ktot and c.N == 4 * roundup(Hd, 8)
    return c


G = [(24, 9, 11, 0, 0)]                          # the 3 x 9 x 11 grid's plain source: M = 297, five stages, the last one partial

GENERIC_CASES = [
    # PLAIN instantiation
    WCase("W0-plain", 0, 3, 9, 11, G, 40),
    WCase("W0-two", 0, 3, 9, 11, _on_grid(9, 11, 24, 16), 40),
    WCase("W0-n136", 0, 3, 9, 11, G, 136, note="second row tile with 8 of 128 rows"),
    WCase("W0-k5", 0, 3, 8, 8, _on_grid(8, 8, 16), 24, ktap=5, pad=2),
    WCase("W0-k7", 0, 3, 8, 8, _on_grid(8, 8, 16), 24, ktap=7, pad=3),
    WCase("W0-slices", 0, 3, 9, 11, G, 40, dys=[(32, 9, 11), (24, 9, 11)], segs=[(0, 16, 0, 8, 1, 0, 0), (16, 32, 1, 0, 1, 0, 0)],
          note="channel slices of two wider tensors; rows [32, 40) are covered by no segment"),
    WCase("W0-pow2-nseg2", 0, 4, 8, 8, _on_grid(8, 8, 24), 40, dys=[(24, 8, 8), (16, 8, 8)],
          segs=[(0, 24, 0, 0, 1, 0, 0), (24, 40, 1, 0, 1, 0, 0)], note="the fast path takes one segment only"),
    # non-PLAIN instantiation
    WCase("W0-pad", 0, 3, 9, 11, TWO_PAD, 40),
    WCase("W0-crop", 0, 3, 9, 11, TWO_CROP, 40),
    _convt("W0-convt16", 16, "all four segments inside one 128-row tile"),
    _convt("W0-convt72", 72, "N = 288: the first 128-row tile spans segments 0 and 1, the second 1, 2 and 3"),
    WCase("W0-s2", 0, 3, 4, 6, [(24, 8, 12, 0, 0)], 40, ktap=2, scale=2, pad=0),
    # ConvLSTM form on a grid that is no power of two
    _lstm("W0-lstm16", 0, 3, 9, 11, 8, 13),
    _lstm("W0-lstm24", 0, 3, 9, 11, 8, 21),
]

P64_CASES = [
    WCase("W1-576", 1, 4, 8, 8, _on_grid(8, 8, 24), 40),
    WCase("W1-two-1152", 1, 4, 8, 8, _on_grid(8, 8, 24, 16), 40),
    WCase("W1-two-k1-128", 1, 4, 8, 8, _on_grid(8, 8, 24, 16), 40, ktap=1, pad=0,
          note="Ktot = 128: every 3x3 Ktot is a multiple of 576, so only a 1x1 gradient reaches the 64 x 256 tile"),
    WCase("W1-c64", 1, 2, 16, 16, _on_grid(16, 16, 64), 64, note="64 -> 64 on a 16-wide image: not the ring kernel"),
    WCase("W1-k1", 1, 2, 16, 16, _on_grid(16, 16, 64), 64, ktap=1, pad=0),
    WCase("W1-small-image", 1, 16, 2, 4, _on_grid(2, 4, 24), 40, note="eight images per 64-pixel stage"),
    _lstm("W1-lstm16", 1, 3, 8, 8, 8, 13),
]

P128_CASES = [
    WCase("W2-128", 2, 2, 16, 16, _on_grid(16, 16, 64), 128),
    WCase("W2-two", 2, 2, 16, 16, _on_grid(16, 16, 64, 64), 72, note="the 128-column tile straddles the sources"),
    WCase("W2-n200", 2, 4, 8, 8, _on_grid(8, 8, 32), 200),
    WCase("W2-k1", 2, 4, 8, 8, _on_grid(8, 8, 72), 136, ktap=1, pad=0),
    _lstm("W2-lstm24", 2, 3, 8, 8, 8, 21),
]

P256_CASES = [
    WCase("W3-one-stage", 3, 4, 4, 4, _on_grid(4, 4, 64), 256),
    WCase("W3-256", 3, 8, 4, 4, _on_grid(4, 4, 256), 256),
    WCase("W3-partial", 3, 1, 32, 32, _on_grid(32, 32, 136), 320, note="partial tiles along rows and columns"),
    WCase("W3-two", 3, 6, 8, 8, _on_grid(8, 8, 72, 200), 264),
]
P256_LONG = WCase("W3-long", 3, 2, 64, 64, _on_grid(64, 64, 64), 256)

# the four ring shapes of test_conv3x3_wgrad; with slab = 0 the ring kernel is not eligible and the descriptor goes to the
# buffer-addressed kernel when H and W are powers of two, else (H = 12) to generic addressing
RING_CASES = [
    WCase("W4-one-strip", 4, 3, 8, 64, _on_grid(8, 64, 64), 64, atomic_shape=1),
    WCase("W4-two-strips", 4, 2, 12, 128, _on_grid(12, 128, 64), 64, atomic_shape=0),
    WCase("W4-two-sources", 4, 2, 8, 128, _on_grid(8, 128, 64, 64), 64, atomic_shape=1),
    WCase("W4-many-tiles", 4, 25, 32, 128, _on_grid(32, 128, 64), 64, atomic_shape=1),
]

PARITY_CASES = GENERIC_CASES + P64_CASES + P128_CASES + P256_CASES
ALL_CASES = PARITY_CASES + [P256_LONG] + RING_CASES
MODE_CASES = {0: "W0-plain", 1: "W1-576", 2: "W2-128", 3: "W3-partial"}       # one case per kernel for the launch modes
FORCED_GENERIC = ["W1-576", "W2-two", "W3-two"]                               # power-of-two cases under UCLSTM_WGRAD_GENERIC=1
# one case per geometry for the CPU test against autograd
AUTOGRAD_CASES = ["W0-plain", "W0-two", "W0-pad", "W0-crop", "W0-convt16", "W0-convt72", "W0-k5", "W0-k7", "W0-s2", "W0-slices",
                  "W0-pow2-nseg2", "W0-lstm24", "W1-lstm16", "W1-k1", "W2-two", "W1-small-image"]


def case(name) -> WCase:
    return next(c for c in ALL_CASES if c.name == name)


# ---------------------------------------------------------------------------------------------
# operands and descriptor
# ---------------------------------------------------------------------------------------------
def make_operands(c: WCase, dtype):
    """Sources [n_img][Hs][Ws][C] and dY tensors [n_img][Hd][Wd][C]: randn * 0.8 rounded to `dtype` on the host."""
    g = torch.Generator().manual_seed(2000 + sum(map(ord, c.name)))
    xs = [(torch.randn(c.n_img, Hs, Ws, Cs, generator=g) * 0.8).to(dtype) for Cs, Hs, Ws, _, _ in c.srcs]
    dys = [(torch.randn(c.n_img, Hd, Wd, Cd, generator=g) * 0.8).to(dtype) for Cd, Hd, Wd in c.dy_tensors()]
    return xs, dys


def case_ref(c: WCase, xs, dys):
    """wgrad_ref of a case on its host operands."""
    return wgrad_ref(c.n_img, c.H, c.W, c.N, c.ktap, c.scale, c.pad, [(x, s[3], s[4]) for x, s in zip(xs, c.srcs)],
                     [(dys[ti], n0, n1, c_off, sc, oy, ox) for n0, n1, ti, c_off, sc, oy, ox in c.segments()])


DUMMY = IC.DUMMY


def build_wgrad_desc(c: WCase, src_ptrs=None, dy_ptrs=None, dwp=None, splits=0, slab=None, overlapped=0, accumulate=0) -> L.WgradDesc:
    """uclstm_wgrad_desc of a case from raw addresses (integers or None: aligned dummies).  slab None: N*Ktot (slab mode)."""
    d = L.WgradDesc()
    d.n_img, d.H, d.W = c.n_img, c.H, c.W
    d.ktap, d.scale, d.pad, d.nsrc = c.ktap, c.scale, c.pad, len(c.srcs)
    for i, (Cs, Hs, Ws, offY, offX) in enumerate(c.srcs):
        s = d.src[i]
        s.ptr = src_ptrs[i] if src_ptrs else DUMMY
        s.C, s.Hs, s.Ws, s.offY, s.offX = Cs, Hs, Ws, offY, offX
    d.N, d.Ktot = c.N, c.Ktot
    segs, tens = c.segments(), c.dy_tensors()
    d.nseg = len(segs)
    for i, (n0, n1, ti, c_off, sc, oy, ox) in enumerate(segs):
        g = d.seg[i]
        g.ptr = dy_ptrs[ti] if dy_ptrs else DUMMY
        g.n_begin, g.n_end, g.c_off, g.scale, g.oy, g.ox = n0, n1, c_off, sc, oy, ox
        g.C, g.Hd, g.Wd = tens[ti]
    d.dwp = dwp
    d.splits, d.accumulate, d.overlapped = splits, accumulate, overlapped
    d.slab = c.N * c.Ktot if slab is None else slab
    return d


def wgrad_shape(d) -> int:
    return int(L.lib.uclstm_igemm_wgrad_shape(C.byref(d)))


def wgrad_splits(d) -> int:
    return int(L.lib.uclstm_igemm_wgrad_splits(C.byref(d)))


def rejected_descriptors():
    """[(what, descriptor)]: a valid case of the table with ONE field broken; the splits query must answer UCLSTM_E_BADARG."""
    def broken(name, fn, **kw):
        d = build_wgrad_desc(case(name), **kw)
        assert wgrad_splits(d) >= 1, name          # the unbroken descriptor is accepted
        fn(d)
        return d

    def set_(field, value):
        return lambda d: setattr(d, field, value)

    c = case("W0-two")
    return [
        ("Ktot inconsistent with the sources", broken("W0-two", set_("Ktot", c.Ktot - 64))),
        ("Ktot of one source only", broken("W0-two", set_("Ktot", 9 * 64))),
        ("N % 8 != 0", broken("W0-plain", set_("N", 36))),
        ("0 < slab < N*Ktot", broken("W0-plain", set_("slab", 40 * 576 - 1))),
        ("nseg 0", broken("W0-plain", set_("nseg", 0))),
        ("nseg 5", broken("W0-plain", set_("nseg", 5))),
        ("misaligned source pointer", broken("W1-576", lambda d: setattr(d.src[0], "ptr", DUMMY + 8))),
        ("misaligned dY pointer", broken("W0-slices", lambda d: setattr(d.seg[1], "ptr", DUMMY + 2))),
        ("ktap 8", broken("W0-k7", lambda d: (setattr(d, "ktap", 8), setattr(d, "Ktot", 64 * 64)))),
        ("segment beyond its tensor's channels", broken("W0-slices", lambda d: setattr(d.seg[0], "c_off", 24))),
    ]
