"""Helpers of tests/test_gpu_boundary_abi.py that need no GPU: f64 references of the module-boundary kernels (layout converters,
first-layer im2col, MaxPool2d(2), OutConv 1x1, SpatialAttention, loss gradient), written from the formulas of include/uclstm.h
with explicit index arithmetic, the case tables, and the input generators.  tests/test_cabi_and_host.py pins every reference to
independent PyTorch code in f64 on the CPU.

The tables hold the smallest shapes at which each path of the kernels in csrc/pointwise.hip and csrc/loss_optim.hip is reached;
every "over the cap" case asserts below that its item count really needs a second trip of the grid-stride loop.
"""
import math

import torch

# launch geometry mirrored from the sources (a case that is meant to wrap the grid-stride loop asserts against these)
NT = 256                               # csrc/pointwise.hip: constexpr int NT, csrc/loss_optim.hip likewise
EW_GRID_CAP = 256 * 8                  # csrc/pointwise.hip ew_grid(): at most 2048 blocks of NT threads
EW_SWEEP = NT * EW_GRID_CAP            # items of one trip of `idx += gridDim.x * NT`: 524 288
LOSS_BWD_GRID_CAP = 2048               # csrc/loss_optim.hip uclstm_loss_bwd: grid_for(total, 2048)
ATTN_GRID_CAP, ATTN_PIX_PER_BLOCK = 4096, 4    # csrc/pointwise.hip uclstm_attention_fwd / _bwd: min((pixels + 3) / 4, 4096) blocks
ATTN_SWEEP = ATTN_GRID_CAP * ATTN_PIX_PER_BLOCK                 # pixels of one trip of attn_desc_kernel / attn_bwd_dpre_kernel
ATTN_LANES = 64                        # attn_desc_kernel: `ch += 64` 16-byte chunks per round of a pixel's wave
OUTCONV_DW_PIX_PER_BLOCK, OUTCONV_DW_BLOCK_CAP = 1024, 1024     # uclstm_outconv_bwd: nb = min(ceil(pixels / 1024), 1024)
OUTCONV_LANES = (2, 4, 8, 16, 32)      # uclstm_outconv_fwd: Cp / 8 with an outconv_fwd_lanes_kernel instance


def manual_seed(*key):
    torch.manual_seed(9000 + sum((i + 1) * 131 * int(k) for i, k in enumerate(key)))


def r16(x, dtype):
    return x.to(dtype).float()


# ---------------------------------------------------------------------------------------------
# layout converters and the first-layer im2col
# ---------------------------------------------------------------------------------------------
# (n_img, C, Cp, H, W, inner): the f32 input is stored [inner][n_img / inner][C][H][W] and output image i reads
# [i % inner][i / inner] (uclstm.h: (i % inner)*outer_stride + (i / inner)*inner_stride); inner = 1 is the plain order,
# inner = B reads [B][T] time-major
LAYOUT_CASES = [
    (3, 5, 8, 7, 9, 1),
    (6, 13, 16, 4, 6, 2),              # [B=2][T=3] time-major, two chunks, C < Cp
    (6, 13, 16, 4, 6, 3),
    (2, 5, 24, 3, 5, 1),               # two chunks of nothing but padding
    (1, 8, 8, 1, 1, 1),
    (4, 1, 8, 1, 13, 1),
    (2, 3, 8, 13, 1, 1),
    (3, 16, 16, 300, 300, 1),          # 540 000 items: second trip of the grid-stride loop
]
LAYOUT_OVER_CAP = [(3, 16, 16, 300, 300, 1)]
# (n_img, C, Cp, H, W): the f32 cell-state pair, Cp free
LAYOUT_F32_CASES = [
    (2, 5, 8, 4, 6),
    (3, 5, 5, 7, 9),
    (1, 1, 3, 1, 1),
    (2, 20, 24, 110, 110),             # to_nhwc: 580 800 items; to_nchw counts C, not Cp: 484 000, one trip only
    (2, 22, 24, 110, 110),             # to_nchw: 532 400 items
]
LAYOUT_F32_OVER_CAP = {"to_nhwc": (2, 20, 24, 110, 110), "to_nchw": (2, 22, 24, 110, 110)}
# (n_img, C, Kp, H, W, inner)
IM2COL_CASES = [
    (6, 2, 24, 6, 5, 2),               # time-major
    (2, 1, 16, 1, 1, 1),
    (2, 3, 32, 1, 7, 1),               # tap boundaries inside a chunk (C = 3, 5, 7), one row / one column
    (2, 3, 32, 7, 1, 1),
    (3, 5, 48, 2, 2, 1),
    (1, 7, 64, 5, 3, 1),
    (4, 2, 24, 216, 216, 1),           # 559 872 items
]
IM2COL_OVER_CAP = [(4, 2, 24, 216, 216, 1)]


def layout_items(case):
    n_img, C, Cp, H, W, _ = case
    return n_img * (Cp // 8) * H * W


def layout_strides(case):
    """(inner, inner_stride, outer_stride) of the C ABI call for a case (C as the channel count of the f32 input)."""
    n_img, C, _, H, W, inner = case
    return inner, C * H * W, (n_img // inner) * C * H * W


def source_image(n_img, inner):
    """Index into the stored image list of the image that output image i reads."""
    i = torch.arange(n_img)
    return (i % inner) * (n_img // inner) + i // inner


def nchw_to_nhwc_ref(x, Cp, inner=1):
    """x [n_img][C][H][W] in storage order -> [n_img][H][W][Cp], channels >= C zero."""
    n_img, C, H, W = x.shape
    out = torch.zeros(n_img, H, W, Cp, dtype=x.dtype)
    src = source_image(n_img, inner)
    for c in range(C):
        out[:, :, :, c] = x[src, c]
    return out


def nhwc_to_nchw_ref(a, C):
    n_img, H, W, _ = a.shape
    out = torch.zeros(n_img, C, H, W, dtype=a.dtype)
    for c in range(C):
        out[:, c] = a[:, :, :, c]
    return out


def im2col_ref(x, Kp, inner=1):
    """out[img][y][x][tap*C + c] = x[img'][c][y + tap/3 - 1][x + tap%3 - 1], zero outside the image and for k >= 9*C."""
    n_img, C, H, W = x.shape
    out = torch.zeros(n_img, H, W, Kp, dtype=x.dtype)
    xs = x[source_image(n_img, inner)]
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if y1 > y0 and x1 > x0:
            for c in range(C):
                out[:, y0:y1, x0:x1, tap * C + c] = xs[:, c, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def layout_specials(dtype):
    """f32 values planted into the inputs of the f32 -> 16-bit converters: signed zeros and infinities, exact half-way points
    between two neighbours of both 16-bit types with an even and an odd lower neighbour, 65520 (the smallest f32 that fp16
    rounds to inf), and subnormals of both types with their half-way points."""
    v = [0.0, -0.0, math.inf, -math.inf, 65520.0, -65520.0, 65504.0, 65519.996]
    for u in (2.0 ** -8, 2.0 ** -11):                       # half a unit of bf16 / fp16 at 1.0
        v += [1.0 + u, 1.0 + 3 * u, -(1.0 + u), -(1.0 + 3 * u), 1.0 + u * (1 + 2.0 ** -10), 1.0 + u * (1 - 2.0 ** -10)]
    v += [2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -26, 1023 * 2.0 ** -24, 2.0 ** -14]   # fp16
    v += [2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, -(2.0 ** -134), 2.0 ** -135, 2.0 ** -126, 2.0 ** -149]  # bf16
    return torch.tensor(v, dtype=torch.float32)


def plant(t, values):
    """values written at a fixed stride through t (flat), the first one at element 0 and one at the last element."""
    f = t.view(-1)
    n = f.numel()
    m = min(n, values.numel())
    f[torch.arange(m) * (n // m)] = values[:m]
    f[n - 1] = values[m - 1]
    return t


def layout_input(case, dtype):
    n_img, C, Cp, H, W, inner = case
    manual_seed(1, n_img, C, Cp, H, W, inner)
    return plant(torch.randn(n_img, C, H, W), layout_specials(dtype))


def stored16_input(shape, dtype):
    """A 16-bit tensor holding random values and every special bit pattern but NaN: zeros, infinities, the extreme normal and
    subnormal values."""
    manual_seed(2, *shape)
    t = torch.randn(*shape).to(dtype)
    tiny = torch.finfo(dtype).smallest_normal
    sp = torch.tensor([0.0, -0.0, math.inf, -math.inf, torch.finfo(dtype).max, -torch.finfo(dtype).max, tiny, tiny / 2, -tiny / 4,
                       tiny * 2.0 ** -7 if dtype == torch.bfloat16 else tiny * 2.0 ** -10], dtype=torch.float64).to(dtype)
    return plant(t, sp)


# ---------------------------------------------------------------------------------------------
# MaxPool2d(2)
# ---------------------------------------------------------------------------------------------
# (n_img, H, W, Cp)
MAXPOOL_CASES = [
    (1, 2, 2, 8),
    (2, 7, 10, 16),                    # odd H: the last row belongs to no window
    (2, 6, 9, 8),                      # odd W
    (3, 5, 5, 24),                     # both odd
    (2, 6, 8, 16),
    (3, 128, 128, 384),                # 589 824 chunks
]
MAXPOOL_OVER_CAP = [(3, 128, 128, 384)]
MAXPOOL_ADD_CASES = [c for c in MAXPOOL_CASES if c[1] % 2 == 0 and c[2] % 2 == 0]


def maxpool_chunks(case):
    n_img, H, W, Cp = case
    return n_img * (H // 2) * (W // 2) * (Cp // 8)


def windows(a):
    """[n_img][H][W][Cp] -> [4][n_img][Ho][Wo][Cp]: the four pixels of every 2x2 window in scan order (0,0) (0,1) (1,0) (1,1)."""
    n_img, H, W, _ = a.shape
    Ho, Wo = H // 2, W // 2
    return torch.stack([a[:, ky:2 * Ho:2, kx:2 * Wo:2] for ky in (0, 1) for kx in (0, 1)])


def maxpool_ref(a):
    """(p, best): the maximum of every window and the scan-order index of its FIRST maximal element (strict '>' replaces)."""
    w = windows(a)
    m, best = w[0].clone(), torch.zeros(w[0].shape, dtype=torch.long)
    for k in (1, 2, 3):
        gt = w[k] > m
        m = torch.where(gt, w[k], m)
        best = torch.where(gt, torch.full_like(best, k), best)
    return m, best


def maxpool_bwd_ref(a, dp, add=None):
    """(da, written): da = add + scatter(dp) to the first maximum; written = the pixels a window covers (uclstm.h: the caller
    zeroes da when H or W is odd, the kernel leaves the trailing row / column alone)."""
    n_img, H, W, Cp = a.shape
    Ho, Wo = H // 2, W // 2
    _, best = maxpool_ref(a)
    da = torch.zeros_like(a) if add is None else add.clone()
    written = torch.zeros(n_img, H, W, dtype=torch.bool)
    for k, (ky, kx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        da[:, ky:2 * Ho:2, kx:2 * Wo:2] += torch.where(best == k, dp, torch.zeros_like(dp))
        written[:, ky:2 * Ho:2, kx:2 * Wo:2] = True
    return da, written


def maxpool_pattern(case):
    """[n_img][Ho][Wo][Cp] int: the planted set of maximal window positions as a bit mask 1..15 (bit k = scan position k), 0 =
    nothing planted.  Runs through all sixteen values along the channels and from window to window."""
    n_img, H, W, Cp = case
    nw = n_img * (H // 2) * (W // 2)
    return ((torch.arange(nw)[:, None] * 7 + torch.arange(Cp)[None, :]) % 16).view(n_img, H // 2, W // 2, Cp)


def maxpool_input(case, dtype):
    """16-bit-representable a [n_img][H][W][Cp] (f32): random values, and in every window / channel with a pattern s != 0 the
    positions of s hold one value above the rest of the window.  Odd windows are negative throughout (top -0.5 over values <= -1),
    even ones hold a positive top over values in [-3, 3]."""
    n_img, H, W, Cp = case
    manual_seed(3, *case)
    a = r16(torch.randn(n_img, H, W, Cp), dtype)
    Ho, Wo = H // 2, W // 2
    pat = maxpool_pattern(case)
    odd = (torch.arange(n_img * Ho * Wo) % 2 == 1).view(n_img, Ho, Wo, 1)
    top_pos = (6.0 + 0.5 * (torch.arange(Cp) % 4)).expand(n_img, Ho, Wo, Cp)
    for k, (ky, kx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        v = a[:, ky:2 * Ho:2, kx:2 * Wo:2]
        rest = torch.where(odd, r16(-v.abs() - 1.0, dtype), v.clamp(-3.0, 3.0))
        top = torch.where(odd, torch.full_like(v, -0.5), top_pos)
        planted = torch.where(((pat >> k) & 1) == 1, top, rest)
        a[:, ky:2 * Ho:2, kx:2 * Wo:2] = torch.where(pat != 0, planted, v)
    assert torch.equal(r16(a, dtype), a)
    return a


# ---------------------------------------------------------------------------------------------
# OutConv 1x1
# ---------------------------------------------------------------------------------------------
# (n_img, HW, C, Cp, Co, bias)
OUTCONV_FWD_CASES = [
    (3, 63, 5, 8, 1, True),            # generic kernel, 1 chunk
    (3, 42, 12, 16, 2, True),          # lanes<2>
    (2, 63, 29, 32, 3, True),          # lanes<4>
    (3, 63, 60, 64, 2, True),          # lanes<8>
    (2, 35, 128, 128, 1, True),        # lanes<16>, C == Cp
    (1, 9, 121, 128, 2, True),         # lanes<16>, C < Cp
    (3, 63, 250, 256, 1, True),        # lanes<32>
    (3, 15, 24, 24, 1, True),          # generic, 3 chunks
    (2, 64, 200, 200, 3, True),        # generic, 25 chunks
    (1, 33, 512, 512, 1, True),        # generic, 64 chunks (`default:`)
    (5, 1, 16, 16, 2, True),           # HW = 1: every pixel its own image
    (2, 63, 29, 32, 3, False),         # bias NULL, lanes
    (3, 15, 24, 24, 1, False),         # bias NULL, generic
    (3, 90000, 12, 16, 1, True),       # lanes<2>: 2048 blocks x 128 pixels = 262 144 < 270 000 pixels
    (2, 270400, 5, 8, 1, True),        # generic: 540 800 pixels
]
OUTCONV_FWD_OVER_CAP = [(3, 90000, 12, 16, 1, True), (2, 270400, 5, 8, 1, True)]
assert {c[3] // 8 for c in OUTCONV_FWD_CASES} == {1, 2, 3, 4, 8, 16, 25, 32, 64}
# input gradient: (n_img, HW, C, Cp, Co, inf planted in dy)
OUTCONV_DA_CASES = [
    (3, 63, 5, 8, 1, False),
    (3, 42, 12, 16, 3, False),
    (3, 15, 24, 24, 1, False),
    (2, 64, 200, 200, 3, False),
    (3, 15, 21, 24, 3, True),          # inf in dy: pad channels exactly zero all the same
    (3, 90000, 12, 16, 1, False),      # 540 000 chunks
]
assert {c[3] // 8 for c in OUTCONV_DA_CASES} == {1, 2, 3, 25} and {c[4] for c in OUTCONV_DA_CASES} == {1, 3}
# parameter gradients with f32 atomics: (n_img, HW, C, Cp, Co)
OUTCONV_DW_CASES = [
    (1, 1, 5, 8, 2),                   # one pixel
    (4, 625, 193, 200, 2),             # 2500 pixels: 3 blocks, the last one ragged; 10 rows x 25 columns = 250 active threads
    (3, 100, 1024, 1024, 1),           # 2 rows x 128 columns
    (3, 100, 2048, 2048, 1),           # 1 row x 256 columns (the most the entry point accepts)
    (1, 1024 * 1024 + 5, 5, 8, 1),     # block count capped at 1024, 1025 pixels per block
]


def outconv_lanes(Cp):
    """Lanes per pixel of the forward kernel uclstm_outconv_fwd runs, 0 for the generic one."""
    return Cp // 8 if Cp // 8 in OUTCONV_LANES else 0


def outconv_fwd_chain(C, Cp):
    """Longest chain of f32 additions of the forward kernel the shape reaches (the n of the (n + 2) * 2^-24 bound)."""
    lanes = outconv_lanes(Cp)
    return 8 + int(math.log2(lanes)) + 1 if lanes else C + 1


def outconv_dw_blocks(pixels):
    return min(-(-pixels // OUTCONV_DW_PIX_PER_BLOCK), OUTCONV_DW_BLOCK_CAP)


def outconv_operands(case, dtype, scale=1.0):
    """a [n_img*HW][Cp] 16-bit-representable with zero pad channels, w [Co][C], b [Co], dy [n_img][Co][HW] (f32; x scale)."""
    n_img, HW, C, Cp, Co = case[:5]
    manual_seed(4, *case[:5])
    a = r16(torch.randn(n_img * HW, Cp), dtype)
    a[:, C:] = 0.0
    away = lambda v, floor: torch.sign(v) * (v.abs() + floor)          # |w * dy| >= 0.01 * scale: no fp16-subnormal da
    return a, away(torch.randn(Co, C) * 0.5, 0.1), torch.randn(Co), away(torch.randn(n_img, Co, HW), 0.1) * scale


def outconv_fwd_ref(a, w, b, n_img, HW):
    """(y [n_img][Co][HW], mag) in f64: y = b + sum_c w[co][c] * a[p][c]; mag = the sum of the magnitudes of those terms."""
    Co, C = w.shape
    a64, w64 = a.double()[:, :C], w.double()
    y, mag = a64 @ w64.t(), a64.abs() @ w64.abs().t()
    if b is not None:
        y, mag = y + b.double(), mag + b.double().abs()
    to_nchw = lambda t: t.view(n_img, HW, Co).permute(0, 2, 1).contiguous()
    return to_nchw(y), to_nchw(mag)


def outconv_bwd_ref(a, w, dy, Cp):
    """f64 (da, da_mag [pixels][Cp]; dw, dw_terms [Co][C]; db, db_terms [Co]) of uclstm.h: da[p][c] = sum_co dy[p][co] * w[co][c]
    (pad channels zero), dw[co][c] = sum_p dy[p][co] * a[p][c], db[co] = sum_p dy[p][co]."""
    n_img, Co, HW = dy.shape
    C = w.shape[1]
    g = dy.double().permute(0, 2, 1).reshape(n_img * HW, Co)
    da, da_mag = torch.zeros(n_img * HW, Cp, dtype=torch.float64), torch.zeros(n_img * HW, Cp, dtype=torch.float64)
    da[:, :C], da_mag[:, :C] = g @ w.double(), g.abs() @ w.double().abs()
    a64 = a.double()[:, :C]
    return da, da_mag, g.t() @ a64, g.abs().t() @ a64.abs(), g.sum(0), g.abs().sum(0)


# ---------------------------------------------------------------------------------------------
# SpatialAttention
# ---------------------------------------------------------------------------------------------
# (n_img, H, W, C, Cp, k)
ATTN_CASES = [
    (1, 1, 1, 1, 8, 1),
    (1, 1, 1, 5, 8, 7),                # the kernel larger than the map: one tap inside
    (3, 1, 9, 21, 24, 7),
    (2, 5, 9, 21, 24, 15),             # widest kernel, wider than the map
    (2, 6, 6, 16, 16, 3),
    (2, 4, 4, 136, 136, 3),
    (2, 4, 4, 1024, 1024, 7),          # 128 chunks: two rounds of the 64-lane channel loop
    (1, 3, 3, 1001, 1008, 3),          # ragged second round, C < Cp; 9 pixels (odd: ddesc starts at the rounded-up offset)
    (2, 17, 19, 8, 8, 7),              # 646 pixels: three blocks of attn_map / attn_bwd_ddesc, three trips of the dw loop
    (5, 64, 64, 3, 8, 5),              # 20 480 pixels: second trip of attn_desc / attn_bwd_dpre
    (3, 64, 64, 512, 512, 3),          # 786 432 chunks: second trip of attn_scale / attn_bwd_dx
]
ATTN_OVER_PIXEL_CAP = [(5, 64, 64, 3, 8, 5)]
ATTN_OVER_CHUNK_CAP = [(3, 64, 64, 512, 512, 3)]
ATTN_TWO_ROUNDS = [(2, 4, 4, 1024, 1024, 7), (1, 3, 3, 1001, 1008, 3)]


def attn_rounds(Cp):
    return -(-(Cp // 8) // ATTN_LANES)


def attn_input(case, dtype):
    """(x [n_img][H][W][Cp] 16-bit-representable f32 with zero pad channels, planted {pixel: (kind, expected arg-max or None)}).  Ties at
    the maximum are planted where the shape has room: two channels of one 16-byte chunk (pixel 0), of two lanes (pixel 1), of two
    rounds of the 64-lane loop (c and c + 512, pixel 2), the first and the last channel (pixel 4); pixel 3 (pixel 0 of a one-pixel
    map) holds only negative valid channels beside zero pad channels when C < Cp."""
    n_img, H, W, C, Cp, k = case
    manual_seed(5, *case)
    pixels = n_img * H * W
    x = torch.randn(pixels, Cp)
    x = r16(torch.sign(x) * (x.abs() + 0.25), dtype)                   # |x| >= 0.25: x * att stays a normal fp16 number
    x[:, C:] = 0.0
    planted = {}

    def tie(pix, chans, kind):
        x[pix, :C] = x[pix, :C].clamp(max=3.0)
        x[pix, list(chans)] = 5.0
        planted[pix] = (kind, min(chans))
    if pixels >= 5:
        if C >= 4:
            tie(0, (1, 3), "one chunk")
        if C >= 12:
            tie(1, (11, 2), "two lanes")
        if C >= 520:
            tie(2, (7 + 512, 7), "two rounds")
        if C >= 9:
            tie(4, (C - 1, 0), "first and last channel")
    if C < Cp:
        pix = 3 if pixels >= 5 else 0
        x[pix, :C] = r16(-x[pix, :C].abs() - 0.5, dtype)
        planted[pix] = ("negative beside zero pads", None)
    assert torch.equal(r16(x, dtype), x)
    return x.view(n_img, H, W, Cp), planted


def attn_weight(case):
    """f32 [2][k][k] conv weight, scaled with 1 / k so that the pre-activation stays within a few units at every k."""
    k = case[5]
    manual_seed(8, *case)
    return torch.randn(2, k, k) * (0.4 / k)


def attn_desc_ref(x, C):
    """(mean, max, first arg-max, sum|x|/C) over the valid channels, f64 / int64 [n_img][H][W]."""
    v = x.double()[..., :C]
    mx = v.max(-1).values
    ch = torch.arange(C).expand(v.shape)
    first = torch.where(v == mx[..., None], ch, torch.full_like(ch, C)).min(-1).values
    return v.sum(-1) / C, mx, first, v.abs().sum(-1) / C


def attn_conv(desc, w, transpose=False):
    """pre[p] = sum_{j,ky,kx} w[j][ky][kx] * desc[p + (ky - r, kx - r)][j] with zero padding (desc [n][H][W][J], w [J][k][k]) and
    the same sum over magnitudes.  transpose: out[q][j] = sum_{ky,kx} w[j][ky][kx] * g[q - (ky - r, kx - r)] (g = desc [n][H][W])."""
    k = w.shape[-1]
    r = k // 2
    n, H, W = desc.shape[:3]
    w = w.double()
    if transpose:
        out, mag = torch.zeros(n, H, W, w.shape[0], dtype=torch.float64), torch.zeros(n, H, W, w.shape[0], dtype=torch.float64)
    else:
        out, mag = torch.zeros(n, H, W, dtype=torch.float64), torch.zeros(n, H, W, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            dy, dx = (r - ky, r - kx) if transpose else (ky - r, kx - r)
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y1 <= y0 or x1 <= x0:
                continue
            s = desc[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            if transpose:
                t = s[..., None] * w[:, ky, kx]
                out[:, y0:y1, x0:x1] += t
                mag[:, y0:y1, x0:x1] += t.abs()
            else:
                t = s * w[:, ky, kx]
                out[:, y0:y1, x0:x1] += t.sum(-1)
                mag[:, y0:y1, x0:x1] += t.abs().sum(-1)
    return out, mag


def attn_fwd_ref(x, w, C):
    """f64 forward of uclstm.h: dict(mean, max, arg, att, pre, out)."""
    mean, mx, arg, _ = attn_desc_ref(x, C)
    pre, _ = attn_conv(torch.stack((mean, mx), -1), w)
    att = 1.0 / (1.0 + torch.exp(-pre))
    return dict(mean=mean, max=mx, arg=arg, pre=pre, att=att, out=x.double() * att[..., None])


def attn_dw_ref(dpre, desc, k):
    """(dw [2][k][k], terms): dw[j][ky][kx] = sum_p dpre[p] * desc[p + (ky - r, kx - r)][j]."""
    r = k // 2
    n, H, W = dpre.shape
    dw, terms = torch.zeros(2, k, k, dtype=torch.float64), torch.zeros(2, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            dy, dx = ky - r, kx - r
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y1 > y0 and x1 > x0:
                t = dpre[:, y0:y1, x0:x1, None] * desc[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
                dw[:, ky, kx], terms[:, ky, kx] = t.sum((0, 1, 2)), t.abs().sum((0, 1, 2))
    return dw, terms


def attn_bwd_ref(x, dout, w, C, fwd):
    """f64 backward of uclstm.h from the forward values in `fwd` (att, mean, max, arg): dict(dpre, ddesc, dw, dx)."""
    x, dout, att = x.double(), dout.double(), fwd["att"]
    dpre = (x * dout).sum(-1) * att * (1.0 - att)
    ddesc, _ = attn_conv(dpre, w, transpose=True)
    dw, _ = attn_dw_ref(dpre, torch.stack((fwd["mean"], fwd["max"]), -1), w.shape[-1])
    onehot = torch.arange(x.shape[-1]) == fwd["arg"][..., None]
    dx = dout * att[..., None] + ddesc[..., 0:1] / C + onehot * ddesc[..., 1:2]
    dx[..., C:] = 0.0
    return dict(dpre=dpre, ddesc=ddesc, dw=dw, dx=dx)


# ---------------------------------------------------------------------------------------------
# loss gradient
# ---------------------------------------------------------------------------------------------
# (planes, H, W)
LOSS_BWD_CASES = [
    (1, 1, 1),
    (2, 1, 7),                         # H = 1 / W = 1: no gradient term at all
    (2, 7, 1),
    (3, 2, 2),
    (3, 8, 8),
    (5, 17, 19),
    (1, 3, 341),
    (9, 256, 257),                     # 592 128 elements
]
LOSS_BWD_OVER_CAP = [(9, 256, 257)]
LOSS_COEFS = (0.37, -1.9)
MASK_VALUES = (0.0, 0.25, 0.5, 1.0)


def loss_input(case, masked):
    """y_pred, y: multiples of 1/64 in [-4, 4] (every difference the kernel takes is exact in f32, so no sign depends on the
    precision); mask drawn from MASK_VALUES or None; every seventh element has y_pred == y, and every eleventh repeats its left
    and upper neighbours' difference, so that sign(0) occurs in all three kinds of term."""
    planes, H, W = case
    manual_seed(6, *case, masked)
    yp = torch.randint(-256, 257, (planes, H, W)).float() / 64
    y = torch.randint(-256, 257, (planes, H, W)).float() / 64
    flat = torch.arange(planes * H * W).view(planes, H, W)
    yp = torch.where(flat % 7 == 3, y, yp)
    d = yp - y
    if W > 1:
        same = (flat % 11 == 5)[:, :, 1:]
        d[:, :, 1:] = torch.where(same, d[:, :, :-1], d[:, :, 1:])
    if H > 1:
        same = (flat % 13 == 6)[:, 1:, :]
        d[:, 1:, :] = torch.where(same, d[:, :-1, :], d[:, 1:, :])
    yp = (y + d).clamp(-4.0, 4.0)
    mask = torch.tensor(MASK_VALUES)[torch.randint(0, 4, (planes, H, W))] if masked else None
    return yp, y, mask


def loss_bwd_ref(yp, y, mask, c1, c2):
    """(grad, bound_mag) in f64 of the closed form
        grad = c1*sign(a-b)*w*m + c2*(-(sx+sy)*m + sx(i,j-1)*m(i,j-1) + sy(i-1,j)*m(i-1,j)),
    w = 1 + 4|b|^3, sx(i,j) = sign((a(i,j+1) - a(i,j)) - (b(i,j+1) - b(i,j))), sy likewise along i, both defined for i < H-1 and
    j < W-1 only; bound_mag = |c1|*w*m + |c2| * the sum of the magnitudes of the four gradient terms."""
    a, b = yp.double(), y.double()
    planes, H, W = a.shape
    m = torch.ones_like(a) if mask is None else mask.double()
    w = 1.0 + 4.0 * b.abs() ** 3
    d = a - b
    sx, sy = torch.zeros_like(a), torch.zeros_like(a)
    if H > 1 and W > 1:
        sx[:, :H - 1, :W - 1] = torch.sign(d[:, :H - 1, 1:] - d[:, :H - 1, :W - 1])
        sy[:, :H - 1, :W - 1] = torch.sign(d[:, 1:, :W - 1] - d[:, :H - 1, :W - 1])
    gg = -(sx + sy) * m
    mag = (sx.abs() + sy.abs()) * m
    gg[:, :, 1:] += (sx * m)[:, :, :-1]
    mag[:, :, 1:] += (sx.abs() * m)[:, :, :-1]
    gg[:, 1:, :] += (sy * m)[:, :-1, :]
    mag[:, 1:, :] += (sy.abs() * m)[:, :-1, :]
    return c1 * torch.sign(d) * w * m + c2 * gg, abs(c1) * w * m + abs(c2) * mag


# ---------------------------------------------------------------------------------------------
# every over-the-cap case needs the trip it is there for
# ---------------------------------------------------------------------------------------------
assert all(layout_items(c) > EW_SWEEP for c in LAYOUT_OVER_CAP + IM2COL_OVER_CAP)
assert LAYOUT_F32_OVER_CAP["to_nhwc"][0] * LAYOUT_F32_OVER_CAP["to_nhwc"][2] * 110 * 110 > EW_SWEEP
assert LAYOUT_F32_OVER_CAP["to_nchw"][0] * LAYOUT_F32_OVER_CAP["to_nchw"][1] * 110 * 110 > EW_SWEEP
assert all(maxpool_chunks(c) > EW_SWEEP for c in MAXPOOL_OVER_CAP)
for _c in OUTCONV_FWD_OVER_CAP:                              # grid = ew_grid(pixels * cpc) blocks of NT / lanes pixels, or ew_grid(pixels)
    _lanes, _pix = outconv_lanes(_c[3]), _c[0] * _c[1]
    assert _pix > (EW_GRID_CAP * (NT // _lanes) if _lanes else EW_SWEEP) and _pix * (_c[3] // 8) > EW_SWEEP
assert {outconv_lanes(c[3]) > 0 for c in OUTCONV_FWD_OVER_CAP} == {True, False}
assert all(c[0] * c[1] * (c[3] // 8) > EW_SWEEP for c in OUTCONV_DA_CASES[-1:])
assert outconv_dw_blocks(OUTCONV_DW_CASES[-1][1]) == OUTCONV_DW_BLOCK_CAP and OUTCONV_DW_CASES[-1][1] > 1024 * 1024
assert all(c[0] * c[1] * c[2] > ATTN_SWEEP for c in ATTN_OVER_PIXEL_CAP)
assert all(c[0] * c[1] * c[2] * (c[4] // 8) > EW_SWEEP for c in ATTN_OVER_CHUNK_CAP)
assert all(attn_rounds(c[4]) == 2 for c in ATTN_TWO_ROUNDS) and max(attn_rounds(c[4]) for c in ATTN_CASES) == 2
assert sum(c[0] * c[1] * c[2] > 256 for c in ATTN_CASES) >= 3 and any((c[0] * c[1] * c[2]) % 2 for c in ATTN_CASES)
assert all(c[0] * c[1] * c[2] > NT * LOSS_BWD_GRID_CAP for c in LOSS_BWD_OVER_CAP)
