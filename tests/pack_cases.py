"""Helpers of tests/test_gpu_pack_abi.py that need no GPU: the index map of a pack descriptor, the references of the weight-panel
kernels of csrc/pack.hip and of uclstm_splitk_finish, the special f32 values, and the case table.  tests/test_pack_cases_host.py
pins the descriptor builders of ops.py to PyTorch's own f64 convolutions and their autograd through these references.

Everything restates include/uclstm.h and nothing else:
  * panel element [n][k] of a descriptor maps to the f32 source element n_ent*stride_n + k_ent*stride_k + tap_eff*stride_tap +
    tapn*stride_ntap (row decode by n_mode, column decode by k_mode, tap_eff = ntaps - 1 - tap when tap_flip), or to nothing;
  * pack: the panel holds the source value rounded to the 16-bit type (round to nearest even) at mapped elements, +0 elsewhere;
  * unpack: grad = (accumulate ? grad : 0) + sum of the slabs, at mapped elements only;
  * bias: bp[n] = b[n_ent] at valid rows, +0 elsewhere;
  * split-K finish: out[p][c] = act16(relu?((sum of slabs + bias[c]) * scale[c] + shift[c])), c < C.

The kernel-family numbers (uclstm_pack_job_init) and the launch geometry below mirror csrc/pack.hip; every case records the family
it was written for and the tests assert it, so a case cannot silently move to another kernel.
"""
import math
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np
import torch

import boundary_cases as BC
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops

# csrc/pack.hip
FAM_GENERIC, FAM_ROWS9, FAM_ROWS4, FAM_TRANS9, FAM_TRANS4 = 0, 1, 2, 3, 4
GENERIC_SWEEP = 256 * 256 * 16          # grid_for(): at most 4096 blocks of 256 threads, one panel element each per trip
ROWS_SLAB_CAP = 64                      # the row-family unpack kernel takes at most 64 slabs; more are folded first
ROWS_CHUNK = 256                        # channels per block of the row family
SENTINEL = 0x5A5A                       # 16-bit pattern of guard elements a kernel must not write


# ---------------------------------------------------------------------------------------------
# index map
# ---------------------------------------------------------------------------------------------
def row_map(d):
    """(valid [N] bool, n_ent [N], tapn [N]) of the descriptor's panel rows (include/uclstm.h: UCLSTM_NMODE_*)."""
    n = np.arange(d.N)
    tapn = np.zeros_like(n)
    if d.n_mode == L.NMODE_IDENTITY:
        n_ent, ok_n = n, n < d.n_valid
    elif d.n_mode == L.NMODE_LSTM:
        hb, gate, j = n >> 6, (n & 63) >> 4, n & 15
        hc = hb * 16 + j
        n_ent, ok_n = gate * d.n_valid + hc, hc < d.n_valid
    else:
        tapn = n // d.n_cp
        n_ent = n - tapn * d.n_cp
        ok_n = n_ent < d.n_valid
    return ok_n, n_ent, tapn


def index_map(d):
    """(valid [N,Ktot] bool, offset [N,Ktot] int64) of the descriptor, straight from include/uclstm.h's definition."""
    K = d.Ktot
    ok_n, n_ent, tapn = (a[:, None] for a in row_map(d))
    k = np.arange(K)[None, :]
    per_tap = d.kseg[0] + d.kseg[1]
    tap = k // per_tap
    kr = k - tap * per_tap
    s = (kr >= d.kseg[0]).astype(np.int64)
    c = np.where(s == 1, kr - d.kseg[0], kr)
    cvalid = np.where(s == 1, d.cvalid[1], d.cvalid[0])
    choff = np.where(s == 1, d.choff[1], d.choff[0])
    if d.k_mode == L.KMODE_IDENTITY:
        ok_k, k_ent = c < cvalid, choff + c
        ntap = d.taps
    elif d.k_mode == L.KMODE_GATES:
        gate, hc = c // d.k_hdp, c % d.k_hdp
        ok_k, k_ent = (gate < 4) & (hc < d.k_hd), choff + gate * d.k_hd + hc
        ntap = d.taps
    else:
        tk = c // d.k_hd
        ok_k, k_ent, tap, ntap = tk < d.k_hdp, c - tk * d.k_hd, tk, d.k_hdp
    tap_eff = (ntap - 1 - tap) if d.tap_flip else tap
    off = n_ent * d.stride_n + k_ent * d.stride_k + tap_eff * d.stride_tap + tapn * d.stride_ntap
    valid = ok_n & ok_k
    return valid, np.where(valid, off, 0)


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def panel_of(d, w, elem_off=0):
    """Panel [N][Ktot] in the dtype of w: w at the mapped positions (w flat, read from element elem_off on), +0 elsewhere."""
    valid, off = index_map(d)
    flat = w.reshape(-1)
    assert int(valid.sum()) > 0 and int((off + elem_off)[valid].max()) < flat.numel()
    v, o = torch.from_numpy(valid), torch.from_numpy(np.where(valid, off + elem_off, 0))
    return torch.where(v, flat[o], torch.zeros((), dtype=w.dtype))


def pack_ref(d, w, elem_off, dtype):
    """uclstm_pack_weights: w.to(dtype) (round to nearest even, NaN stays NaN) at mapped positions, +0 elsewhere."""
    return panel_of(d, w.float(), elem_off).to(dtype)


def unpack_ref(d, slabs, base, accumulate):
    """uclstm_unpack_wgrad in f64.  slabs [nslab][N][Ktot], base the flat previous gradient.  Returns (ref, mag, mapped), all
    flat over the gradient: ref = (accumulate ? base : 0) + sum of slabs where the map reaches (base elsewhere: untouched), mag =
    sum|slab terms| + |base if accumulate|, mapped = the elements the map reaches.  The map must reach no element twice."""
    valid, off = index_map(d)
    o = off[valid]
    assert np.unique(o).size == o.size, "two panel elements map to one gradient element"
    tot = slabs.sum(0, dtype=torch.float64).numpy()[valid]
    mag = slabs.abs().sum(0, dtype=torch.float64).numpy()[valid]
    b = base.double().numpy().reshape(-1)
    ref, m, mapped = b.copy(), np.zeros_like(b), np.zeros(b.size, bool)
    mapped[o] = True
    ref[o] = (b[o] if accumulate else 0.0) + tot
    m[o] = mag + (np.abs(b[o]) if accumulate else 0.0)
    return ref, m, mapped


def ordered_unpack_f32(d, slabs, base, accumulate, groups=1):
    """The f32 association of the ordered unpack (header): one group -- t = s0; t += s1; ...; out = (accumulate ? base : 0) + t;
    several groups of per = ceil(nslab / G) -- every group's sum starts from 0, out = (accumulate ? base : 0) + g0 + g1 + ...,
    left to right.  Returns (gradient flat f32 with base at unmapped elements, scratch [G][N*Ktot] f32 or None)."""
    valid, off = index_map(d)
    valid, off = valid.ravel(), off.ravel()
    sl = slabs.numpy().reshape(slabs.shape[0], -1)
    nslab = sl.shape[0]
    out = base.numpy().reshape(-1).astype(np.float32).copy()
    start = out[off[valid]] if accumulate else np.zeros(int(valid.sum()), np.float32)
    if groups == 1:
        t = sl[0].copy()
        for s in range(1, nslab):
            t = t + sl[s]
        out[off[valid]] = start + t[valid]
        return out, None
    per = -(-nslab // groups)
    scratch = np.zeros((groups, sl.shape[1]), np.float32)
    for g in range(groups):
        for s in range(g * per, min(nslab, (g + 1) * per)):
            scratch[g] = scratch[g] + sl[s]
    scratch[:, ~valid] = 0.0
    acc = start
    for g in range(groups):
        acc = acc + scratch[g][valid]
    out[off[valid]] = acc
    return out, scratch


def bias_ref(d, b):
    """uclstm_pack_bias: bp[n] = b[n_ent] at valid rows (under every tap of a tap-major panel), +0 elsewhere; dtype of b."""
    ok_n, n_ent, _ = row_map(d)
    assert int(n_ent[ok_n].max()) < b.numel()
    ok, ne = torch.from_numpy(ok_n), torch.from_numpy(np.where(ok_n, n_ent, 0))
    return torch.where(ok, b.reshape(-1)[ne], torch.zeros((), dtype=b.dtype))


def bias_len(d):
    return d.n_valid * (4 if d.n_mode == L.NMODE_LSTM else 1)


def splitk_finish_ref(pre, bias, scale, shift, relu, C):
    """uclstm_splitk_finish in f64.  pre [nslab][pixels][ld]; bias / scale / shift [C] or None.  Returns (ref, mag) [pixels][C],
    mag = (sum|slabs| + |bias|) * |scale| + |shift|, the magnitude of the terms before they cancel."""
    p = pre.double()[:, :, :C]
    s, a = p.sum(0), p.abs().sum(0)
    if bias is not None:
        s, a = s + bias.double(), a + bias.double().abs()
    if scale is not None:
        s, a = s * scale.double(), a * scale.double().abs()
    if shift is not None:
        s, a = s + shift.double(), a + shift.double().abs()
    if relu:
        s = s.clamp(min=0.0)
    return s, a


# ---------------------------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------------------------
F32_MAX = 3.4028234663852886e38


def specials(dtype):
    """boundary_cases.layout_specials (signed zeros, infinities, half-way points of both parities, the fp16 overflow threshold,
    16-bit subnormals) + NaN, the largest finite f32 (rounds to inf in both types) and an f32 subnormal above bf16's smallest."""
    return torch.cat((BC.layout_specials(dtype), torch.tensor([math.nan, F32_MAX, -F32_MAX, 2.0 ** -127, -3 * 2.0 ** -130], dtype=torch.float32)))


def weight_with_specials(case, dtype):
    """The case's f32 weight: randn with the special values planted at a fixed stride."""
    BC.manual_seed(31, *case.wshape, case.elem_off)
    return BC.plant(torch.randn(case.wshape), specials(dtype))


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
@dataclass
class PackCase:
    name: str
    make: Callable[[], "L.PackDesc"]
    wshape: Tuple[int, ...]
    family: int                       # what uclstm_pack_job_init must report
    elem_off: int = 0
    unpack: bool = False              # a descriptor the host layer passes to uclstm_unpack_wgrad
    note: str = ""

    @property
    def desc(self):
        return self.make()


def conv_fwd(Co, cs):
    return ops.conv_pack_desc(Co, sum(cs), list(cs), [ops.cpad(c) for c in cs])


def conv2x2_dgrad_desc(Co, Ci):
    """Input-gradient panel of a 2x2 convolution with weight [Co][Ci][2][2]: rows = input channels, K = (flipped tap, output
    channel).  Filled by hand: no layer of the model needs it, but uclstm_pack_weights routes it to the transposed 4-tap kernel."""
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = ops.cpad(Ci), 4, 1
    d.kseg[0], d.kseg[1] = ops.kseg(ops.cpad(Co)), 0
    d.cvalid[0], d.cvalid[1] = Co, 0
    d.choff[0] = d.choff[1] = 0
    d.Ktot = 4 * d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, Ci, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 1
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = 4, Ci * 4, 1, 0
    return d


def _lstm_w(Hd, Cx, k=3):
    return (4 * Hd, Cx + Hd, k, k)


CASES = [
    # rows family, 9 taps
    PackCase("conv fwd c255", lambda: conv_fwd(8, [255]), (8, 255, 3, 3), FAM_ROWS9, unpack=True, note="one chunk, last channel padding"),
    PackCase("conv fwd c256", lambda: conv_fwd(8, [256]), (8, 256, 3, 3), FAM_ROWS9, unpack=True, note="one full chunk"),
    PackCase("conv fwd c257", lambda: conv_fwd(8, [257]), (8, 257, 3, 3), FAM_ROWS9, unpack=True, note="second chunk holds one channel"),
    PackCase("conv fwd 264+24", lambda: conv_fwd(8, [264, 24]), (8, 288, 3, 3), FAM_ROWS9, unpack=True,
             note="two chunks, then a 64-column segment holding 24 channels"),
    PackCase("lstm fwd hd5", lambda: ops.lstm_pack_desc(5, 3), _lstm_w(5, 3), FAM_ROWS9, note="pad rows inside a 16-row gate block"),
    PackCase("lstm x half hd5", lambda: ops.lstm_half_pack_desc(5, 3, "x"), _lstm_w(5, 3), FAM_ROWS9),
    PackCase("lstm h half hd5", lambda: ops.lstm_half_pack_desc(5, 3, "h"), _lstm_w(5, 3), FAM_ROWS9),
    PackCase("lstm fwd hd40", lambda: ops.lstm_pack_desc(40, 24), _lstm_w(40, 24), FAM_ROWS9),
    PackCase("lstm x half hd40", lambda: ops.lstm_half_pack_desc(40, 24, "x"), _lstm_w(40, 24), FAM_ROWS9),
    PackCase("lstm h half hd40", lambda: ops.lstm_half_pack_desc(40, 24, "h"), _lstm_w(40, 24), FAM_ROWS9, note="choff != 0"),
    PackCase("lstm wgrad hd5", lambda: ops.lstm_wgrad_unpack_desc(5, 3), _lstm_w(5, 3), FAM_ROWS9, unpack=True),
    PackCase("lstm wgrad hd40", lambda: ops.lstm_wgrad_unpack_desc(40, 24), _lstm_w(40, 24), FAM_ROWS9, unpack=True),
    # rows family, 4 taps
    PackCase("convT dgrad 48x24", lambda: ops.convt_dgrad_pack_desc(48, 24), (48, 24, 2, 2), FAM_ROWS4),
    PackCase("convT dgrad ci20", lambda: ops.convt_dgrad_pack_desc(20, 24), (20, 24, 2, 2), FAM_ROWS4, note="N = 24 > n_valid"),
    # transposed family, 9 taps
    PackCase("conv dgrad cs20", lambda: ops.conv_dgrad_pack_desc(72, 44, 20), (72, 44, 3, 3), FAM_TRANS9,
             note="N = 24: the second 16-row block is half empty, rows 20..23 zero"),
    PackCase("conv dgrad second source", lambda: ops.conv_dgrad_pack_desc(72, 44, 24), (72, 44, 3, 3), FAM_TRANS9, elem_off=20 * 9),
    PackCase("lstm dgrad x hd5", lambda: ops.lstm_dgrad_pack_desc(5, 3, 3), _lstm_w(5, 3), FAM_TRANS9,
             note="4 * Hd_p = 32 < kseg: gate boundaries inside one 64-column block, columns of 'gates' 4..7 padding"),
    PackCase("lstm dgrad h hd5", lambda: ops.lstm_dgrad_pack_desc(5, 3, 5), _lstm_w(5, 3), FAM_TRANS9, elem_off=3 * 9),
    PackCase("lstm dgrad x hd40", lambda: ops.lstm_dgrad_pack_desc(40, 24, 24), _lstm_w(40, 24), FAM_TRANS9, note="kseg 192, columns 160..191 padding"),
    PackCase("lstm dgrad h hd40", lambda: ops.lstm_dgrad_pack_desc(40, 24, 40), _lstm_w(40, 24), FAM_TRANS9, elem_off=24 * 9),
    # transposed family, 4 taps
    PackCase("conv2x2 dgrad", lambda: conv2x2_dgrad_desc(24, 20), (24, 20, 2, 2), FAM_TRANS4),
    # generic family
    PackCase("convT fwd co24", lambda: ops.convt_pack_desc(48, 24), (48, 24, 2, 2), FAM_GENERIC, unpack=True),
    PackCase("convT fwd co20", lambda: ops.convt_pack_desc(48, 20), (48, 20, 2, 2), FAM_GENERIC, unpack=True),
    PackCase("first layer ci1", lambda: ops.im2col_pack_desc(24, 1, 16), (24, 1, 3, 3), FAM_GENERIC, unpack=True),
    PackCase("first layer ci2", lambda: ops.im2col_pack_desc(24, 2, 24), (24, 2, 3, 3), FAM_GENERIC, unpack=True),
    PackCase("first layer ci3", lambda: ops.im2col_pack_desc(24, 3, 32), (24, 3, 3, 3), FAM_GENERIC, unpack=True),
    PackCase("lstm 1x1", lambda: ops.lstm_pack_desc(16, 8, 1), _lstm_w(16, 8, 1), FAM_GENERIC),
    PackCase("lstm 5x5", lambda: ops.lstm_pack_desc(5, 3, 5), _lstm_w(5, 3, 5), FAM_GENERIC),
    PackCase("lstm 7x7", lambda: ops.lstm_pack_desc(5, 3, 7), _lstm_w(5, 3, 7), FAM_GENERIC),
    PackCase("lstm 7x7 two trips", lambda: ops.lstm_pack_desc(48, 24, 7), _lstm_w(48, 24, 7), FAM_GENERIC,
             note="192 x 6272 = 1 204 224 elements: second trip of the generic grid-stride loop"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
UNPACK_CASES = [c for c in CASES if c.unpack]
OVER_SWEEP = "lstm 7x7 two trips"


def expected_blocks(d, family):
    """nblocks uclstm_pack_job_init must fill in (header: gx * rows for the staged families, the capped element grid otherwise)."""
    if family in (FAM_ROWS9, FAM_ROWS4):
        return (-(-d.kseg[0] // ROWS_CHUNK) + -(-d.kseg[1] // ROWS_CHUNK)) * d.N
    if family in (FAM_TRANS9, FAM_TRANS4):
        return -(-(d.kseg[0] + d.kseg[1]) // 64) * -(-d.N // 16)
    return min(-(-d.N * d.Ktot // 256), GENERIC_SWEEP // 256)


def unpack_path(d, family, nslab, slab, dwp_addr):
    """Which kernel uclstm_unpack_wgrad runs, from the preconditions stated in csrc/pack.hip: 'rows' (row-family kernel, at most 64
    slabs), 'fold' (more slabs, folded into slab 0 first -- needs slab and N*Ktot multiples of 4 floats and a 16-byte aligned dwp),
    'generic' (one thread per element) otherwise."""
    if family in (FAM_ROWS9, FAM_ROWS4):
        if nslab <= ROWS_SLAB_CAP:
            return "rows"
        if slab % 4 == 0 and (d.N * d.Ktot) % 4 == 0 and dwp_addr % 16 == 0:
            return "fold"
    return "generic"


def generic_groups(d, nslab):
    """Slab groups of the one-thread-per-element unpack (header: 1 .. 1024, a function of descriptor and slab count): with at
    least 16 slabs and fewer than 512 blocks of 256 elements, min(1024 / blocks, nslab / 4) groups, at least 1."""
    gx = min(-(-d.N * d.Ktot // 256), GENERIC_SWEEP // 256)
    if nslab >= 16 and gx < 512:
        return max(1, min(1024 // gx, nslab // 4))
    return 1


def ordered_groups(d, family, nslab):
    """uclstm_unpack_wgrad_ordered_groups: 1 for row-family descriptors (row kernel or fold; every panel of the table has
    N*Ktot % 4 == 0), generic_groups otherwise."""
    if family in (FAM_ROWS9, FAM_ROWS4) and (nslab <= ROWS_SLAB_CAP or (d.N * d.Ktot) % 4 == 0):
        return 1
    return generic_groups(d, nslab)


# uclstm_splitk_finish: (pixels, C, ld, nslab, slab_extra, relu, (bias, scale, shift) present)
SPLITK_CASES = (
    [(37, 24, 24, ns, 0, 1, (True, True, True)) for ns in (1, 2, 3, 8)] +
    [(37, 24, 28, 3, 0, 1, (True, True, True)),            # ld = C + 4: NaN in the pad columns
     (37, 24, 28, 2, 8, 0, (True, True, True)),            # slab > pixels * ld, no ReLU
     (5, 8, 8, 2, 0, 0, (True, True, True)),
     (3, 512, 512, 3, 4, 1, (True, True, True)),
     (3, 512, 516, 2, 0, 0, (True, True, True))] +
    [(11, 8, 12, 2, 4, r, (b, s, h)) for r in (0, 1) for b in (False, True) for s in (False, True) for h in (False, True)] +
    [(8200, 512, 512, 2, 0, 1, (True, True, True))]        # 524 800 chunks: second trip of the grid-stride loop
)
SPLITK_OVER_CAP = (8200, 512, 512, 2, 0, 1, (True, True, True))
assert SPLITK_OVER_CAP[0] * (SPLITK_OVER_CAP[1] // 8) > BC.EW_SWEEP


def splitk_input(case, dtype):
    """(pre [nslab][slab] f32 flat per slab with NaN in the pad columns and the gap, bias, scale, shift).  Values stay in the
    normal range of fp16: |result| well above 2^-14 is not guaranteed per element, so check_elementwise's own assertion decides."""
    pixels, C, ld, nslab, extra, relu, (hb, hs, hh) = case
    BC.manual_seed(77, pixels, C, ld, nslab, extra, relu, hb, hs, hh)
    slab = pixels * ld + extra
    pre = torch.full((nslab, slab), math.nan)
    body = torch.randn(nslab, pixels, C)
    pre[:, :pixels * ld].view(nslab, pixels, ld)[:, :, :C] = body
    bias = torch.randn(C) if hb else None
    scale = (torch.rand(C) + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0) if hs else None
    shift = torch.randn(C) * 0.5 if hh else None
    return pre, body, bias, scale, shift
