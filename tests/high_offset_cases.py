"""Helpers of tests/test_gpu_high_offset.py that need no GPU: the case table of the GEMM families at the top of the 2 GiB range
of a 32-bit buffer descriptor, the integer data generator, and the rules that choose which images a test looks at.
tests/test_high_offset_cases_host.py checks all of it with dummy pointers.

Both families address an operand through a buffer descriptor in which bit 31 of the byte offset means "outside the tensor"
(csrc/igemm_fwd.hip, csrc/igemm_wgrad.hip), so a launch admits operands of just under 2 GiB.  Every case here takes the smallest
image its kernel admits and the LARGEST image count the library's own launch conditions admit; `over` is what the shape query
must answer for one more image (UCLSTM_E_BADARG or the kernel the launch re-routes to).  The image counts are not written down:
fwd_max_images / wgrad_fast_max_images / wgrad_max_images restate the conditions of plan_fwd and wgrad_run, and the host test
asserts that the library accepts the count and refuses (re-routes) the next.

The operands are a pure integer function of (image, pixel, channel, salt) with values k / 8, |k| <= 7: exact in bf16 and in
fp16, computed by the same torch code on the device for a whole tensor and on the host for any image.  The function is an
affine map modulo 2^31 (odd multiplier on the image index) followed by two bijective mixing rounds, so two addresses that
differ by 2^30, 2^31 or 2^32 bytes (a whole number of images in every case) hold different 31-bit states and unrelated values.

What a test looks at:
  * per-pixel kernels: every element of the images of sampled_units(): the first and last unit, the units holding byte offsets
    2^30 and 2^31 - 2^23 of every operand, the unit of the last tile, both sides of every launch cut handed in, and seeded
    draws up to 16 units.  A unit is one BatchNorm group (one image when the case has no statistics).
  * weight gradients: dY is zero outside whole-image windows -- the same selection plus both sides of every pixel-range
    boundary of the uclstm_igemm_wgrad_splits() plan -- X is dense, and the f64 reference sums the windows only.
"""
import ctypes as C
import dataclasses
import random
from dataclasses import dataclass
from typing import Optional

import torch

import igemm_cases as IC
import wgrad_cases as WC
from igemm_cases import Case
from wgrad_cases import WCase

L = IC.L
E_BADARG = -1
DESC_LIMIT = (1 << 31) - (1 << 22)       # bytes (+ bias) of an operand of the forward family and of the fast weight-gradient paths
WGRAD_ELEMS = (1 << 31) - (1 << 20)      # elements of an operand of the weight-gradient family (generic addressing)
OFFSETS = (1 << 30, (1 << 31) - (1 << 23))
M31 = (1 << 31) - 1


# ---------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------
def values(imgs, pixels, ch, salt, device="cpu"):
    """int64 [len(imgs)][pixels][ch] in [-7, 7]: the operand's value * 8 at (image, pixel, channel)."""
    i = torch.as_tensor(imgs, dtype=torch.int64, device=device).view(-1, 1, 1)
    p = torch.arange(pixels, dtype=torch.int64, device=device).view(1, -1, 1)
    c = torch.arange(ch, dtype=torch.int64, device=device).view(1, 1, -1)
    x = (i * 1000003 + p * 8191 + c * 131 + salt * 7919) & M31
    x = (x * 1103515245 + 12345) & M31
    x ^= x >> 15
    x = (x * 69069 + 1) & M31
    x ^= x >> 13
    return x % 15 - 7


def host_images(imgs, Hs, Ws, ch, salt, dtype):
    """[len(imgs)][Hs][Ws][ch] of `dtype` on the host."""
    return (values(imgs, Hs * Ws, ch, salt).to(torch.float32) / 8).to(dtype).view(len(imgs), Hs, Ws, ch)


def fill(t, salt, img0=0, chunk_elems=1 << 25):
    """Write the generator into t [n][Hs][Ws][ch] (any float dtype, on its own device) for images img0 ..; int64 temporaries of
    at most chunk_elems elements."""
    n, Hs, Ws, ch = t.shape
    step = max(1, chunk_elems // (Hs * Ws * ch))
    for a in range(0, n, step):
        b = min(n, a + step)
        v = values(torch.arange(img0 + a, img0 + b, device=t.device), Hs * Ws, ch, salt, t.device)
        t[a:b] = (v.to(torch.float32) / 8).view(b - a, Hs, Ws, ch)


# ---------------------------------------------------------------------------------------------
# launch conditions, restated from the code
# ---------------------------------------------------------------------------------------------
def fwd_bias(src, pad):
    """plan_fwd: the descriptor bias of a source, 2 * (max(pad + offY, 0) * Ws + max(pad + offX, 0) + 1) * C bytes."""
    Cs, _, Ws, offY, offX = src
    return 2 * (max(pad + offY, 0) * Ws + max(pad + offX, 0) + 1) * Cs


def fwd_max_images(srcs, pad):
    """plan_fwd: the largest n_img with n_img * Hs * Ws * C * 2 + bias < 2^31 - 2^22 for every source."""
    return min((DESC_LIMIT - fwd_bias(s, pad) - 1) // (s[1] * s[2] * s[0] * 2) for s in srcs)


def wgrad_fast_max_images(c: WCase):
    """wgrad_run, fast paths: dY bytes < 2^31 - 2^22 and source bytes + (Ws + 1) * C * 2 < 2^31 - 2^22; the ring kernel
    (wgrad_c64_ok) asks n_img * H * W * 128 < 2^31 - 2^22 of its 64-channel operands, which is the first of the two."""
    n = min((DESC_LIMIT - 1) // (c.H * c.W * Cd * 2) for Cd, _, _ in c.dy_tensors())
    return min([n] + [(DESC_LIMIT - (s[2] + 1) * s[0] * 2 - 1) // (c.H * c.W * s[0] * 2) for s in c.srcs])


def wgrad_max_images(c: WCase):
    """wgrad_run: every operand holds fewer than 2^31 - 2^20 ELEMENTS."""
    per = [s[0] * s[1] * s[2] for s in c.srcs] + [Cd * Hd * Wd for Cd, Hd, Wd in c.dy_tensors()]
    return min((WGRAD_ELEMS - 1) // p for p in per)


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
@dataclass
class HCase:
    name: str
    case: object                     # igemm_cases.Case or wgrad_cases.WCase, n_img at its limit
    over: int                        # the shape query's answer for one more unit
    note: str = ""
    walk: Optional[bool] = None      # 256 x 256 weight gradient: with / without the valid-pixel walk

    @property
    def unit(self):
        """Images per BatchNorm group (1 without statistics): what `one more` adds."""
        c = self.case
        return c.n_img // c.groups if isinstance(c, Case) and c.stats else 1

    def with_images(self, n):
        c = self.case
        if isinstance(c, Case):
            return dataclasses.replace(c, n_img=n, groups=n // self.unit if c.stats else 1)
        return dataclasses.replace(c, n_img=n)


def _g(H, W, *cs):
    return [(c, H, W, 0, 0) for c in cs]


def _fwd(name, shape, srcs, N, H=16, W=16, note="", **kw):
    n = fwd_max_images(srcs, kw.get("pad", 1))
    stats = kw.pop("stats", False)
    return HCase(name, Case(name, shape, n, H, W, srcs, N, groups=n if stats else 1, stats=stats, **kw), E_BADARG, note)


def _lstm(name, shape, Cx, Hd, H=16, W=16):
    c = IC._lstm(name, shape, 1, H, W, Cx, Hd, ())
    return HCase(name, dataclasses.replace(c, n_img=fwd_max_images(c.srcs, 1)), E_BADARG)


def _wfast(name, shape, srcs, N, H=16, W=16, note="", walk=None, **kw):
    c = WCase(name, shape, 1, H, W, srcs, N, **kw)
    return HCase(name, dataclasses.replace(c, n_img=wgrad_fast_max_images(c)), 0, note, walk)


def _wgeneric(name, srcs, N, H, W, note=""):
    c = WCase(name, 0, 1, H, W, srcs, N)
    return HCase(name, dataclasses.replace(c, n_img=wgrad_max_images(c)), E_BADARG, note)


SHIFTED = [(64, 16, 16, 0, 0), (64, 16, 16, 1, 1)]       # second source one pixel down and right: the largest bias of a 16-wide image

STORE_CASES = [
    _fwd("HF0-n160", 0, _g(16, 16, 64), 160, stats=True, note="64 -> 160: the destination crosses 2^31 and 2^32 bytes"),
    _fwd("HF0-shifted", 0, SHIFTED, 72, note="two sources, the second with offY = offX = 1"),
    _fwd("HF1", 1, _g(16, 16, 64), 64, stats=True),
    _fwd("HF2-tile", 2, _g(16, 16, 64, 64), 128, stats=True, note="patch loop, 256 consecutive pixels per tile"),
    _fwd("HF2-strip", 2, _g(4, 128, 128), 128, H=4, W=128, stats=True, note="patch loop, 4 x 64 strip tiles"),
    _fwd("HF3-ring", 3, _g(4, 64, 64), 64, H=4, W=64, stats=True),
    _fwd("HF4-k1-n128", 4, _g(16, 16, 64), 128, ktap=1, pad=0, stats=True, note="64 -> 128: the destination crosses 2^31 bytes"),
    _fwd("HF4-tap2", 4, _g(32, 32, 64), 128, ktap=2, scale=2, pad=0, note="ktap 2 / scale 2 gather of the transposed conv"),
]
LSTM_PATCH, LSTM_TAP = _lstm("HL2", 2, 64, 64), _lstm("HL0", 0, 24, 64)
SLAB_PATCH = _fwd("HA2", 2, _g(16, 16, 64, 64), 72, epi=L.EPI_ATOMIC, ksplit=2, bias=False)
SLAB_TAP = _fwd("HA0", 0, _g(16, 16, 24, 64), 72, epi=L.EPI_ATOMIC, ksplit=2, bias=False)
FWD_CASES = STORE_CASES + [LSTM_PATCH, LSTM_TAP, SLAB_PATCH, SLAB_TAP]
GROUP_PATCH, GROUP_TAP = [LSTM_PATCH, SLAB_PATCH], [LSTM_TAP, SLAB_TAP]       # uclstm_igemm_fwd_group / _group_tap

WGRAD_CASES = [
    _wgeneric("HW0-generic", _g(12, 12, 64), 64, 12, 12, note="12 x 12: generic by geometry, operands of 4 GiB less 2 MiB"),
    _wgeneric("HW0-beyond", _g(16, 16, 64), 64, 16, 16, note="power-of-two image beyond the fast path's byte range: generic by size"),
    _wfast("HW1", 1, _g(16, 16, 64), 64),
    _wfast("HW2", 2, _g(16, 16, 128), 128),
    _wfast("HW3-dense", 3, _g(16, 16, 192), 256, walk=False, note="192 K columns per tap: tiles straddle taps, no walk"),
    _wfast("HW3-walk", 3, _g(16, 16, 256), 256, walk=True),
    _wfast("HW4-ring", 4, _g(4, 64, 64), 64, H=4, W=64, atomic_shape=1),
]
FP16_CASES = ["HF2-tile", "HW1"]         # the addressing is shared between the two builds: one case per family

ALL = {h.name: h for h in FWD_CASES + WGRAD_CASES}


def fwd_shape(c: Case):
    d = IC.dummy_desc(c)
    return int(L.lib.uclstm_igemm_fwd_shape(C.byref(d)))


def wgrad_plan(c: WCase, slab=None):
    """(kernel, pixel ranges) of the automatic plan in slab mode."""
    d = WC.build_wgrad_desc(c, slab=slab)
    return WC.wgrad_shape(d), WC.wgrad_splits(d)


def walks(c: WCase):
    """wgrad_run's `vw`: a 256 x 256 launch of a 3x3 / pad 1 gradient whose K tiles each belong to one tap."""
    return c.N >= 256 and c.ktap == 3 and c.pad == 1 and sum(c.ksegs) % 256 == 0 and c.M < (1 << 24) - 4096


# ---------------------------------------------------------------------------------------------
# which images a test looks at
# ---------------------------------------------------------------------------------------------
def operand_bytes_per_image(c):
    """Bytes per image of every 16-bit operand a launch of the case addresses through a buffer descriptor."""
    per = [s[0] * s[1] * s[2] * 2 for s in c.srcs]
    if isinstance(c, WCase):
        per += [Cd * Hd * Wd * 2 for Cd, Hd, Wd in c.dy_tensors()]
    return per


def required_images(c):
    """{what: image}: first, last, the images holding byte offsets 2^30 and 2^31 - 2^23 of each operand, the last tile's image."""
    req = {"first": 0, "last": c.n_img - 1, "last tile": (c.M - 1) // (c.H * c.W)}
    for k, per in enumerate(operand_bytes_per_image(c)):
        for off in OFFSETS:
            if off < c.n_img * per:
                req[f"operand {k} byte {off}"] = off // per
    return req


def sampled_units(c, unit=1, cuts=(), count=16, seed=0):
    """Sorted unit indices (a unit is `unit` consecutive images): the units of required_images(), the units on both sides of
    every image index in `cuts`, and seeded draws up to `count`."""
    n_units = c.n_img // unit
    s = {i // unit for i in required_images(c).values()}
    for cut in cuts:
        s |= {u for u in ((cut - 1) // unit, cut // unit) if 0 <= u < n_units}
    rng = random.Random(1234 + seed + sum(map(ord, c.name)))
    while len(s) < min(count, n_units):
        s.add(rng.randrange(n_units))
    return sorted(s)


def unit_images(units, unit):
    return [u * unit + k for u in units for k in range(unit)]


def ring_block_cuts(c, blocks=256, keep=(1, 2, 128, 255)):
    """Image indices at which a persistent block of the ring kernels hands over to the next (blocks of ceil(tiles / blocks)
    consecutive 4 x 64 tiles, numbered image-major); the cuts after blocks `keep` only: every block runs the same code."""
    tiles_per_img = (c.H // 4) * (c.W // 64)
    tiles = c.n_img * tiles_per_img
    per = -(-tiles // min(tiles, blocks))
    return sorted({min(c.n_img - 1, k * per // tiles_per_img) for k in keep if k * per < tiles})


def wgrad_boundary_images(h: HCase, splits):
    """Image indices holding a pixel-range boundary of a `splits`-range plan.  wgrad_run cuts the M pixels (the valid-pixel
    walk: the n_img * hv * wv entries of each tap's walk, with the same range length) into ranges of
    roundup(ceil(M / splits), 64); the ring kernel gives each of its `splits` blocks ceil(tiles / splits) whole tiles."""
    c = h.case
    if c.shape == 4:
        tiles_per_img = (c.H // 4) * (c.W // 64)
        per = -(-c.n_img * tiles_per_img // splits)
        return sorted({k * per // tiles_per_img for k in range(1, splits) if k * per < c.n_img * tiles_per_img})
    chunk = IC.roundup(-(-c.M // splits), 64)
    per_img = {c.H * c.W}
    if h.walk:
        per_img |= {(c.H - 1) * c.W, c.H * (c.W - 1), (c.H - 1) * (c.W - 1)}
    return sorted({k * chunk // p for p in per_img for k in range(1, splits) if k * chunk // p < c.n_img})


def wgrad_windows(h: HCase, splits, cuts=()):
    """Sorted window images of a weight-gradient case under a `splits`-range plan."""
    return sampled_units(h.case, 1, tuple(wgrad_boundary_images(h, splits)) + tuple(cuts))


# ---------------------------------------------------------------------------------------------
# f64 references on the images a test looks at
# ---------------------------------------------------------------------------------------------
SALT_X, SALT_DY, SALT_C = 1, 11, 21      # sources are SALT_X + index, dY tensors SALT_DY + index


def fwd_sources(c: Case, imgs, dtype):
    """[(x [len(imgs)][Hs][Ws][C] host, offY, offX)] of the images, as gather_a takes them (images are independent)."""
    return [(host_images(imgs, Hs, Ws, Cs, SALT_X + k, dtype), offY, offX) for k, (Cs, Hs, Ws, offY, offX) in enumerate(c.srcs)]


def fwd_a(c: Case, imgs, dtype):
    return IC.gather_a(len(imgs), c.H, c.W, c.ktap, c.scale, c.pad, fwd_sources(c, imgs, dtype))


def wgrad_window_ref(c: WCase, windows, dtype, batch=16):
    """(dWp, mag) [N][Ktot] in f64 of dY = generator inside the window images, zero elsewhere: the sum over the windows."""
    ref = torch.zeros(c.N, c.Ktot, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for a in range(0, len(windows), batch):
        imgs = windows[a:a + batch]
        xs = [(host_images(imgs, Hs, Ws, Cs, SALT_X + k, dtype), offY, offX) for k, (Cs, Hs, Ws, offY, offX) in enumerate(c.srcs)]
        dys = [host_images(imgs, Hd, Wd, Cd, SALT_DY + k, dtype) for k, (Cd, Hd, Wd) in enumerate(c.dy_tensors())]
        r, m = WC.wgrad_ref(len(imgs), c.H, c.W, c.N, c.ktap, c.scale, c.pad, xs,
                            [(dys[ti], n0, n1, c_off, sc, oy, ox) for n0, n1, ti, c_off, sc, oy, ox in c.segments()])
        ref += r
        mag += m
    return ref, mag
