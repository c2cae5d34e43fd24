"""The fused BatchNorm kernels, the ConvLSTM point-wise kernels and the BatchNorm statistics kernels, each called directly
at the C ABI and compared with the same formulas in f64 on the CPU, on the same 16-bit-rounded inputs.

The module tests reach these kernels through whole modules at one or two friendly shapes and 1e-2 .. 3e-2 tolerances; a block ->
pixel mapping that drops the tail of a group, a lane reduction of the wrong width, a missing split-K slab or a wrong arg-max tie
rule is a few per cent there and O(1) here.  Shapes are the smallest that reach every path of each block plan: every lane count,
C < Cp, ragged groups, unroll tails, capped block counts with empty trailing blocks, non-power-of-two window decodes.

Bounds (those of test_bn_bwd_reduce_and_apply_against_f64_at_the_c_abi in test_gpu_ops.py):
  * reductions                     max |err| / sum|terms| <= 2e-6
  * 16-bit element-wise outputs    |err| <= u16 * 1.01 * |ref| + 2^-21 * mag + 1e-30, u16 = half a unit in the last place
                                   (2^-8 bf16, 2^-11 fp16), mag = sum of the magnitudes of the terms before they cancel
  * f32 atomics over blocks        (2e-6 + nblocks * 2^-24) * sum|terms|   (one f32 rounding per atomic add)
Output buffers are pre-filled with NaN, no element is left out of a comparison, and wherever a reference needs the STORED
activation a = act16(relu(z*scale + shift)) it takes the kernel's own (f32 and f64 can land on different sides of a 16-bit
rounding boundary), which is itself checked against f64 to half a unit.

fp16 runs the backward kernels on gradients x 1024, as fp16 training does (include/uclstm.h: loss scaling keeps fp16 gradients out
of the subnormal range, where the spacing 2^-24 is no longer relative to the value); each fp16 check asserts that no reference
value it bounds is subnormal unless the f32 term of its bound covers half that spacing.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
F16_MIN_NORMAL, F16_HALF_SPACING = 2.0 ** -14, 2.0 ** -25


def u16(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def loss_scale(dtype):
    return 1.0 if dtype == torch.bfloat16 else 1024.0


def tag(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def r16(x, dtype):
    """x rounded to the 16-bit type (round to nearest even, as the kernels' conversions), held in f32."""
    return x.to(dtype).float()


def dev16(x, dtype):
    return x.to(dtype).to(DEV).contiguous()


def dev32(x):
    return x.float().to(DEV).contiguous()


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def call(K, name, *args):
    U._lib.check(getattr(K, name)(*args, ops._stream()), name)


def bn_params(groups, Cp, C):
    """scale / shift / mean / rstd [groups][Cp] f32; negative scale on every third channel (the mask is on z*scale + shift, not
    on z); all four are zero on the pad channels c >= C, as the statistics kernels leave them."""
    scale, shift = torch.rand(groups, Cp) + 0.5, torch.randn(groups, Cp) * 0.5
    scale[:, ::3] *= -1.0
    mean, rstd = torch.randn(groups, Cp) * 0.3, torch.rand(groups, Cp) + 0.5
    for t in (scale, shift, mean, rstd):
        t[:, C:] = 0.0
    return scale, shift, mean, rstd


def draw_z(gi, scale, shift, dtype):
    """16-bit z [pixels][Cp], re-drawn wherever the f64 pre-activation z*scale + shift lies within 1e-4 of zero."""
    sc, sh = scale.double()[gi], shift.double()[gi]
    z = r16(torch.randn(sc.shape), dtype)
    for _ in range(50):
        near = ((z.double() * sc + sh).abs() < 1e-4) & (sc != 0)
        n = int(near.sum())
        if n == 0:
            break
        z[near] = r16(torch.randn(n), dtype)
    return z


def preactivation(z, gi, scale, shift):
    """f64 z*scale + shift, after asserting that the ReLU mask cannot depend on f32 versus f64 evaluation: no pre-activation within
    1e-4 of zero (on pad channels scale = shift = 0 and it is exactly zero in any precision)."""
    sc, sh = scale.double()[gi], shift.double()[gi]
    y = z.double() * sc + sh
    assert bool(((y.abs() >= 1e-4) | ((sc == 0) & (sh == 0))).all())
    return y


def assert_f16_bound_attainable(ref, f32_term, dtype, what):
    if dtype == torch.float16:
        sub = (ref != 0) & (ref.abs() < F16_MIN_NORMAL)
        assert bool((f32_term[sub] >= F16_HALF_SPACING).all()), f"{what}: the inputs give subnormal fp16 results the bound cannot hold"


def check_elementwise(got, ref, mag, dtype, what, f32_units=2.0 ** -21):
    """|got - ref| <= u16 * 1.01 * |ref| + f32_units * mag + 1e-30 at every element (got must be finite everywhere)."""
    got = got.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: elements not written"
    assert_f16_bound_attainable(ref, f32_units * mag, dtype, what)
    d = (got - ref).abs()
    bound = u16(dtype) * 1.01 * ref.abs() + f32_units * mag + 1e-30
    worst = float((d / bound).max())
    print(f"[parity] {what}: worst |err| / bound {worst:.3f} (<= 1), max |err| {float(d.max()):.3e} over {d.numel()} elements")
    bad = int((d > bound).sum())
    assert bad == 0, f"{what}: {bad} of {d.numel()} elements beyond half a 16-bit unit + f32 rounding (worst {worst:.3f} x the bound)"
    return worst


def check_sums(got, ref, terms, what, tol=2e-6):
    """max |got - ref| / sum|terms| <= tol."""
    got = got.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: elements not written"
    e = float(((got - ref).abs() / (terms + 1e-30)).max())
    print(f"[parity] {what}: max |err| / sum|terms| {e:.2e} (<= {tol:.2e})")
    assert e <= tol, f"{what}: {e:.3e} > {tol:.3e}"
    return e


def bn_backward_reference(y64, z, da, gi, n, scale, mean, rstd, groups):
    """g_, xhat and the f64 sums of the header's formulas: s1 = sum g_, s2 = sum g_*xhat over the pixels of a group, g_ = da where
    z*scale + shift > 0; also the sums of magnitudes (the scale of f32 summation error)."""
    Cp = z.shape[1]
    g0 = torch.where(y64 > 0, da.double(), torch.zeros_like(y64))
    xhat = (z.double() - mean.double()[gi]) * rstd.double()[gi]
    s1 = g0.view(groups, n, Cp).sum(1)
    s2 = (g0 * xhat).view(groups, n, Cp).sum(1)
    a1 = g0.abs().view(groups, n, Cp).sum(1)
    a2 = (g0 * xhat).abs().view(groups, n, Cp).sum(1)
    return g0, xhat, torch.stack((s1, s2), -1), torch.stack((a1, a2), -1)


def dz_reference(g0, xhat, z, gi, n, scale, mean, rstd, sums):
    """dz = scale*(g_ - s1/n - xhat*s2/n) with the sums the apply kernel was given (the kernel's own f32 results), and the magnitude
    of the regrouped form the kernels evaluate: scale*g_ + k1*z + k0, k1 = -scale*rstd*s2/n, k0 = -scale*s1/n - k1*mean."""
    k1s, k2s = sums[..., 0][gi], sums[..., 1][gi]
    sc = scale.double()[gi]
    ref = sc * (g0 - k1s / n - xhat * k2s / n)
    k1 = (scale.double() * rstd.double())[gi].abs() * k2s.abs() / n
    mag = sc.abs() * (g0.abs() + k1s.abs() / n) + k1 * (z.double().abs() + mean.double()[gi].abs())
    return ref, mag


# ---------------------------------------------------------------------------------------------
# 1. MaxPool2d(2) fused into the BatchNorm stage: uclstm_bn_apply_relu_pool / uclstm_bn_pool_bwd_reduce / _apply
# ---------------------------------------------------------------------------------------------
# (n_img, H, W, Cp, groups)
POOL_SHAPES = [
    (2, 2, 2, 8, 2),              # one window per group
    (3, 6, 10, 24, 3),            # Wo = 5, Ho = 3 (window decode by non-powers of two); 85 rows x 3 lanes = 255 active threads
    (4, 14, 6, 64, 2),            # 42 windows per group, 2 blocks of 21: a block ends inside an image
    (2, 2, 66, 8, 1),             # 66 windows per group, 3 blocks of 22
    (6, 10, 10, 136, 3),          # 17 lanes per pixel, 15 rows
    (1100, 20, 20, 8, 1100),      # cap 4096 / 1100 = 3 blocks per group of 34 windows, the last one ragged
    (2, 4, 4, 2048, 2),           # one row per sweep
    (2, 700, 400, 8, 1),          # 140000 windows per group, capped at 4096 blocks of 35: the last 96 blocks are empty
]


def pool_blocks_per_group(shape):
    n_img, H, W, Cp, groups = shape
    wpg = (n_img // groups) * (H // 2) * (W // 2)
    return min((wpg + 31) // 32, max(1, 4096 // groups))


def to_windows(t, n_img, H, W):
    """[n_img*H*W][Cp] -> [windows][4][Cp], the four pixels of a 2x2 window in scan order."""
    Cp = t.shape[-1]
    return t.view(n_img, H // 2, 2, W // 2, 2, Cp).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4, Cp)


def from_windows(w, n_img, H, W):
    Cp = w.shape[-1]
    return w.view(n_img, H // 2, W // 2, 2, 2, Cp).permute(0, 1, 3, 2, 4, 5).reshape(-1, Cp)


def pool_inputs(shape, dtype):
    n_img, H, W, Cp, groups = shape
    torch.manual_seed(7000 + n_img + 3 * H + 5 * W + Cp)
    C, cpc = Cp - 3, Cp // 8
    n = (n_img // groups) * H * W                     # pixels per group
    pixels, nw = n_img * H * W, n_img * (H // 2) * (W // 2)
    gi = torch.arange(pixels) // n
    scale, shift, mean, rstd = bn_params(groups, Cp, C)
    z = draw_z(gi, scale, shift, dtype)
    # ties: in one window in eight per channel chunk, the z of one pixel of the window is copied into a later pixel of it (same
    # image, so same group: the copy has the pre-activation of its source and cannot land on the ReLU kink).  The source pixel is
    # first made the window's positive maximum on every live channel -- z = sign(scale) * max(max|z| of the window + 0.5,
    # (|shift| + 0.5) / |scale|), so its pre-activation exceeds the other pixels' and 0.49 -- which makes every such tie one at a
    # positive maximum by construction, not by the luck of the draw (the smallest shape has two windows)
    zw = to_windows(z, n_img, H, W).view(nw, 4, cpc, 8)
    sel = ((torch.arange(nw)[:, None] + torch.arange(cpc)[None, :]) % 8) == 0
    src = torch.randint(0, 3, (nw, cpc))
    dst = (src + 1 + (torch.rand(nw, cpc) * (3 - src)).long()).clamp(max=3)
    assert bool(((dst > src) & (dst <= 3)).all())
    gw = torch.arange(nw) // ((n_img // groups) * (H // 2) * (W // 2))                     # group of a window
    scw, shw = scale[gw].view(nw, cpc, 8), shift[gw].view(nw, cpc, 8)
    top = torch.maximum(zw.abs().amax(1) + 0.5, (shw.abs() + 0.5) / scw.abs().clamp(min=0.25))
    top = r16(torch.sign(scw) * top, dtype)                                                 # pad channels (scale 0): z = 0
    boosted = zw.scatter(1, src[:, None, :, None].expand(nw, 1, cpc, 8), top[:, None])
    zw = torch.where(sel[:, None, :, None], boosted, zw)
    val = zw.gather(1, src[:, None, :, None].expand(nw, 1, cpc, 8))
    tied = zw.scatter(1, dst[:, None, :, None].expand(nw, 1, cpc, 8), val)
    z = from_windows(torch.where(sel[:, None, :, None], tied, zw).reshape(nw, 4, Cp), n_img, H, W).contiguous()
    y64 = preactivation(z, gi, scale, shift)
    S = loss_scale(dtype)
    dp = r16(S * (torch.randn(nw, Cp) + 1.0), dtype)
    dskip = r16(S * (torch.randn(pixels, Cp) + 1.0), dtype)
    return dict(n=n, C=C, pixels=pixels, nw=nw, gi=gi, scale=scale, shift=shift, mean=mean, rstd=rstd, z=z, y64=y64, dp=dp, dskip=dskip)


@functools.lru_cache(maxsize=1)
def pool_case(shape, dtype):
    """Inputs of one pool case and the forward kernels' outputs on them (shared by the cases of a shape)."""
    n_img, H, W, Cp, groups = shape
    c = pool_inputs(shape, dtype)
    K = U._lib.kernels(dtype)
    zd = dev16(c["z"], dtype)
    par = [dev32(c[k]) for k in ("scale", "shift", "mean", "rstd")]
    a, a_plain, p = nan_like((c["pixels"], Cp), dtype), nan_like((c["pixels"], Cp), dtype), nan_like((c["nw"], Cp), dtype)
    call(K, "uclstm_bn_apply_relu_pool", ops._p(zd), ops._p(a), ops._p(p), ops._p(par[0]), ops._p(par[1]), n_img, H, W, Cp, groups)
    call(K, "uclstm_bn_apply_relu", ops._p(zd), ops._p(a_plain), ops._p(par[0]), ops._p(par[1]), c["pixels"], c["n"], Cp)
    return dict(c, zd=zd, par=par, a=a.float().cpu(), a_plain=a_plain.float().cpu(), p=p.float().cpu())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=str)
def test_bn_apply_relu_pool_against_f64(shape, dtype):
    """a = act16(relu(z*scale + shift)) within half a unit of f64 and bit-identical to uclstm_bn_apply_relu, p exactly the 2x2 maximum
    of the returned a, pad channels zero."""
    n_img, H, W, Cp, groups = shape
    c = pool_case(shape, dtype)
    a, p = c["a"], c["p"]
    ref = c["y64"].clamp(min=0.0)
    mag = (c["z"].double() * c["scale"].double()[c["gi"]]).abs() + c["shift"].double()[c["gi"]].abs()
    check_elementwise(a, ref, mag, dtype, f"bn_apply_relu_pool a {shape} {tag(dtype)}", f32_units=2.0 ** -22)
    assert torch.equal(a, c["a_plain"]), "stored activation differs from uclstm_bn_apply_relu"
    assert bool(torch.isfinite(p).all())
    aw = to_windows(a, n_img, H, W)
    assert torch.equal(p, aw.max(1).values), "pooled tensor is not the 2x2 maximum of the stored activation"
    assert bool((a[:, c["C"]:] == 0).all()) and bool((p[:, c["C"]:] == 0).all())
    m = aw.max(1, keepdim=True).values
    ties = (((aw == m).sum(1) >= 2) & (m[:, 0] > 0)).any(1).float().mean().item()
    print(f"[parity] bn_apply_relu_pool {shape} {tag(dtype)}: {ties:.1%} of the windows hold a tie at a positive maximum")
    assert ties >= 0.05


@pytest.mark.parametrize("use_skip", [True, False], ids=["dskip", "noskip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=str)
def test_bn_pool_bwd_reduce_and_apply_against_f64(shape, use_skip, dtype):
    """da = act16(dskip + scatter(dp)) (or the plain scatter) to the first maximum of the stored activation in scan order, strict
    '>', then the BatchNorm backward sums and dz of the header's formulas."""
    n_img, H, W, Cp, groups = shape
    c = pool_case(shape, dtype)
    n, gi, scale, mean, rstd, z = c["n"], c["gi"], c["scale"], c["mean"], c["rstd"], c["z"]
    aw = to_windows(c["a"], n_img, H, W)
    is_max = aw == aw.max(1, keepdim=True).values
    first = is_max & (is_max.cumsum(1) == 1)                       # first maximum in scan order
    scat = torch.where(first, c["dp"][:, None, :].expand_as(aw), torch.zeros_like(aw))
    da = from_windows(scat, n_img, H, W)
    if use_skip:
        da = r16(c["dskip"] + da, dtype)                            # one IEEE f32 addition, rounded to 16 bits: exact
    g0, xhat, s_ref, s_abs = bn_backward_reference(c["y64"], z, da, gi, n, scale, mean, rstd, groups)

    K = U._lib.kernels(dtype)
    rows = int(U._lib.lib.uclstm_bn_pool_bwd_rows(n_img, H, W, Cp, groups))
    assert rows > 0 and rows % groups == 0 and rows // groups == pool_blocks_per_group(shape)
    dpd = dev16(c["dp"], dtype)
    dsd = dev16(c["dskip"], dtype) if use_skip else None
    partials, sums = nan_like((rows, Cp, 2), torch.float32), nan_like((groups, Cp, 2), torch.float32)
    call(K, "uclstm_bn_pool_bwd_reduce", ops._p(c["zd"]), ops._p(dsd), ops._p(dpd), *[ops._p(t) for t in c["par"]], ops._p(partials),
         ops._p(sums), n_img, H, W, Cp, groups)
    what = f"{shape} {'dskip' if use_skip else 'noskip'} {tag(dtype)} ({rows // groups} blocks per group)"
    got = sums.cpu()
    check_sums(got, s_ref, s_abs, f"bn_pool_bwd_reduce {what}")

    dz = nan_like((c["pixels"], Cp), dtype)
    call(K, "uclstm_bn_pool_bwd_apply", ops._p(c["zd"]), ops._p(dsd), ops._p(dpd), *[ops._p(t) for t in c["par"]], ops._p(sums), ops._p(dz),
         n_img, H, W, Cp, groups)
    ref, mag = dz_reference(g0, xhat, z, gi, n, scale, mean, rstd, got.double())
    check_elementwise(dz.float().cpu(), ref, mag, dtype, f"bn_pool_bwd_apply {what}")


# ---------------------------------------------------------------------------------------------
# 2. Output head fused into the last BatchNorm stage: uclstm_bn_head_fwd / _bwd_reduce / _bwd_apply
# ---------------------------------------------------------------------------------------------
# (pixels per group, groups, Cp, C)
HEAD_SHAPES = [
    (131, 3, 64, 64),             # ragged group
    (7, 1100, 8, 5),              # group smaller than one sweep; block cap reached
    (333, 2, 16, 9),              # 2 lanes, C < Cp
    (50, 3, 32, 17),              # 4 lanes, C < Cp
    (5000, 1, 128, 100),          # 16 lanes, C < Cp
    (777, 2, 256, 256),           # 32 lanes, ragged group
    (1000, 2, 512, 509),          # 64 lanes: a whole wave per pixel
    (40000, 1, 8, 8),             # reduce capped at 1024 blocks of 40 pixels: blocks 1000 .. 1023 are empty
    (40960, 2, 64, 64),           # many blocks
]


@functools.lru_cache(maxsize=1)
def head_case(shape, dtype):
    ppg, groups, Cp, C = shape
    torch.manual_seed(8000 + ppg + 7 * Cp + C)
    pixels = ppg * groups
    gi = torch.arange(pixels) // ppg
    scale, shift, mean, rstd = bn_params(groups, Cp, Cp)           # every channel live: only w says which ones count
    z = draw_z(gi, scale, shift, dtype)
    y64 = preactivation(z, gi, scale, shift)
    w = (torch.rand(Cp) + 0.5) * (torch.randint(0, 2, (Cp,)).float() * 2 - 1)
    w[C:] = float("nan")                                            # must never reach a result
    b = torch.randn(1) * 0.5
    dy = (loss_scale(dtype) * (torch.randn(pixels) + 1.0)).float()
    K = U._lib.kernels(dtype)
    zd = dev16(z, dtype)
    par = [dev32(t) for t in (scale, shift, mean, rstd)]
    a = nan_like((pixels, Cp), dtype)
    call(K, "uclstm_bn_apply_relu", ops._p(zd), ops._p(a), ops._p(par[0]), ops._p(par[1]), pixels, ppg, Cp)
    a = a.float().cpu()
    # the stored activation the references below take as an input, itself against f64 to half a unit
    mag = (z.double() * scale.double()[gi]).abs() + shift.double()[gi].abs()
    check_elementwise(a, y64.clamp(min=0.0), mag, dtype, f"bn_apply_relu a {shape} {tag(dtype)}", f32_units=2.0 ** -22)
    return dict(pixels=pixels, gi=gi, scale=scale, shift=shift, mean=mean, rstd=rstd, z=z, y64=y64, w=w, b=b, dy=dy, zd=zd, par=par, a=a,
                wd=dev32(w), bd=dev32(b), dyd=dev32(dy))


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=str)
def test_bn_head_fwd_against_f64(shape, dtype):
    """y[p] = b + sum_{c < C} w[c] * a[p][c], with and without the bias; w is NaN beyond C."""
    ppg, groups, Cp, C = shape
    c = head_case(shape, dtype)
    K = U._lib.kernels(dtype)
    terms = c["a"].double()[:, :C] * c["w"].double()[:C]
    for bias in (c["b"], None):
        b64 = 0.0 if bias is None else float(bias)
        y = nan_like((c["pixels"],), torch.float32)
        call(K, "uclstm_bn_head_fwd", ops._p(c["zd"]), ops._p(c["par"][0]), ops._p(c["par"][1]), ops._p(c["wd"]),
             None if bias is None else ops._p(c["bd"]), ops._p(y), c["pixels"], ppg, Cp, C)
        check_sums(y.cpu(), terms.sum(1) + b64, terms.abs().sum(1) + abs(b64),
                   f"bn_head_fwd {shape} {tag(dtype)} {'no bias' if bias is None else 'bias'}")


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=str)
def test_bn_head_bwd_reduce_and_apply_against_f64(shape, dtype):
    """da[p][c] = act16(dy[p] * w[c]) formed on the fly (zero beyond C): the BatchNorm backward sums, dw / db (f32 atomics over
    the blocks, zeroed by the caller, dw untouched beyond C) and dz."""
    ppg, groups, Cp, C = shape
    c = head_case(shape, dtype)
    gi, scale, mean, rstd, z, dy = c["gi"], c["scale"], c["mean"], c["rstd"], c["z"], c["dy"]
    w0 = torch.where(torch.arange(Cp) < C, c["w"], torch.zeros(Cp))
    da = r16(dy[:, None] * w0[None, :], dtype)                      # one IEEE f32 multiplication, rounded to 16 bits: exact
    g0, xhat, s_ref, s_abs = bn_backward_reference(c["y64"], z, da, gi, ppg, scale, mean, rstd, groups)
    wterms = dy.double()[:, None] * c["a"].double()[:, :C]

    K = U._lib.kernels(dtype)
    rows = int(U._lib.lib.uclstm_bn_bwd_reduce_rows(c["pixels"], ppg))
    assert rows >= groups and rows % groups == 0
    partials, sums = nan_like((rows, Cp, 2), torch.float32), nan_like((groups, Cp, 2), torch.float32)
    dw = torch.zeros(Cp, device=DEV)
    dw[C:] = 12345.0
    db = torch.zeros(1, device=DEV)
    call(K, "uclstm_bn_head_bwd_reduce", ops._p(c["zd"]), ops._p(c["dyd"]), *[ops._p(t) for t in c["par"]], ops._p(c["wd"]), ops._p(partials),
         ops._p(sums), ops._p(dw), ops._p(db), c["pixels"], ppg, Cp, C)
    what = f"{shape} {tag(dtype)} ({rows // groups} blocks per group)"
    got = sums.cpu()
    check_sums(got, s_ref, s_abs, f"bn_head_bwd_reduce sums {what}")
    atomic = 2e-6 + rows * 2.0 ** -24
    dwc = dw.cpu()
    check_sums(dwc[:C], wterms.sum(0), wterms.abs().sum(0), f"bn_head_bwd_reduce dw {what}", tol=atomic)
    check_sums(db.cpu(), dy.double().sum().view(1), dy.double().abs().sum().view(1), f"bn_head_bwd_reduce db {what}", tol=atomic)
    assert bool((dwc[C:] == 12345.0).all()), "dw written beyond C"

    dz = nan_like((c["pixels"], Cp), dtype)
    call(K, "uclstm_bn_head_bwd_apply", ops._p(c["zd"]), ops._p(c["dyd"]), *[ops._p(t) for t in c["par"]], ops._p(sums), ops._p(c["wd"]),
         ops._p(dz), c["pixels"], ppg, Cp, C)
    ref, mag = dz_reference(g0, xhat, z, gi, ppg, scale, mean, rstd, got.double())
    check_elementwise(dz.float().cpu(), ref, mag, dtype, f"bn_head_bwd_apply {what}")


# ---------------------------------------------------------------------------------------------
# 3. uclstm_lstm_bwd_pointwise
# ---------------------------------------------------------------------------------------------
# (pixels, Hd_p)
LSTM_BWD_SHAPES = [
    (1, 8),
    (77, 24),                     # Hd_p not a power of two
    (300, 64),
    (5, 520),                     # 65 chunks per pixel
    (9000, 512),                  # 576000 chunks > 2048 blocks x 256 threads: the grid-stride loop wraps
]
# (name, dh_a given, dh_b form: None | "16" | "f32", slabs, dh_b_is_f32, dc_is_zero, c_prev given)
LSTM_BWD_OPTIONS = [
    ("dh_a only, dc zero, no c_prev", True, None, 0, 0, 1, False),
    ("dh_b 16-bit", True, "16", 0, 0, 0, True),
    ("dh_b f32 one slab, no dh_a", False, "f32", 1, 1, 0, True),
    ("dh_b f32 three slabs", True, "f32", 3, 1, 0, True),
    ("dh_b f32 three slabs consumed", True, "f32", 3, 2, 0, True),
]
# The relative error of the kernel's f32 evaluation (its tanh is 1 - 2 / (__expf(2x) + 1)) in units of `mag`, the magnitude of the
# terms before they cancel.  Measured on MI355X as the largest |err| / mag of dc_io over every case of
# test_lstm_bwd_pointwise_against_f64: 3.581e-07 (ROCm 7.2 hipcc, 50 cases).  E = 4 x the measured
# value, never above 2^-16.
LSTM_BWD_E = min(4 * 3.581e-07, 2.0 ** -16)
GAP = 1.0e30                      # between the slabs of dh_b (slab stride > pixels * Hd_p): never to be read or written


def signed_away_from_zero(shape, lo, hi):
    return (torch.rand(shape) * (hi - lo) + lo) * (torch.randint(0, 2, shape).float() * 2 - 1)


@functools.lru_cache(maxsize=1)
def lstm_bwd_case(shape, dtype):
    """Post-activation gates i, f, o in (0, 1), g in (-1, 1), rounded to 16 bits; |c| up to 4 (tanh saturates in part of the tensor).
    bf16: the whole range -- gates are sigmoid(3 x normal) and tanh(2 x normal), so a good part is saturated (up to the largest
    value below 1, 1 - 2^-8), c_prev uniform in (-4, 4), gradients normal.
    fp16: gradients x the loss scale, and gates in [0.1, 0.9], |g| in [0.1, 0.9], |c_prev| >= 0.1, |dh terms| >= 0.25 x the loss
    scale: a gate gradient is a product of up to five of these factors, and it must stay a normal fp16 number (or mag >= 2^-25 / E)
    for the relative bound to be one that a correctly rounded result can hold.  Saturated gates are therefore not run in fp16;
    the arithmetic in front of the final conversion is the same f32 code in both builds."""
    pixels, Hd = shape
    torch.manual_seed(9000 + pixels + Hd)
    S = loss_scale(dtype)
    if dtype == torch.float16:
        gates = torch.rand(pixels, 4, Hd) * 0.8 + 0.1
        gates[:, 2] = signed_away_from_zero((pixels, Hd), 0.1, 0.9)
        gates = r16(gates, dtype)
        c_prev = signed_away_from_zero((pixels, Hd), 0.1, 4.0).float()
        dh_a = r16(S * signed_away_from_zero((pixels, Hd), 0.25, 2.0), dtype)
        dh_b16 = r16(S * signed_away_from_zero((pixels, Hd), 0.25, 2.0), dtype)
        slabs = (S * signed_away_from_zero((3, pixels, Hd), 0.25, 2.0)).float()
    else:
        below_one = 1.0 - 2.0 ** -8
        gates = torch.sigmoid(3.0 * torch.randn(pixels, 4, Hd))
        gates[:, 2] = torch.tanh(2.0 * torch.randn(pixels, Hd))
        gates = r16(gates, dtype).clamp(min=-below_one, max=below_one)
        assert bool((gates[:, [0, 1, 3]] > 0).all())
        assert pixels * Hd < 10000 or float((gates[:, 0] == below_one).float().mean()) > 1e-3         # saturated gates are there
        c_prev = (torch.rand(pixels, Hd) * 8 - 4).float()
        dh_a, dh_b16 = r16(torch.randn(pixels, Hd), dtype), r16(torch.randn(pixels, Hd), dtype)
        slabs = torch.randn(3, pixels, Hd)
    c_new = (torch.rand(pixels, Hd) * 8 - 4).float()
    dc = (S * torch.randn(pixels, Hd)).float()
    return dict(gates=gates, c_new=c_new, c_prev=c_prev, dc=dc, dh_a=dh_a, dh_b16=dh_b16, slabs=slabs,
                gates_d=dev16(gates, dtype), c_new_d=dev32(c_new), c_prev_d=dev32(c_prev), dh_a_d=dev16(dh_a, dtype))


@pytest.mark.parametrize("option", LSTM_BWD_OPTIONS, ids=lambda o: o[0].replace(" ", "_").replace(",", ""))
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", LSTM_BWD_SHAPES, ids=str)
def test_lstm_bwd_pointwise_against_f64(shape, option, dtype):
    """The header's formulas in f64 with exact tanh:  dh = dh_a + dh_b (all slabs);  tc = tanh(c_new);  do = dh*tc*o*(1-o);
    dc' = dc + dh*o*(1-tc^2);  df = dc'*c_prev*f*(1-f);  di = dc'*g*i*(1-i);  dg = dc'*i*(1-g^2);  dc_io <- dc'*f.
    Bounds: dgates u16*1.01*|ref| + E*mag, dc_io E*mag, with mag = (|dc| + sum|dh terms|*o) x the gate factor of the output
    (|g|*i*(1-i), |c_prev|*f*(1-f), i*(1+g^2), f; for do: sum|dh terms|*o*(1-o), tanh being O(1) with an absolute error).
    A missing slab, a cleared wrong slab or a dropped term is O(1) x mag.
    E = 4 x 3.581e-07, the largest |err| / mag of dc_io measured over all 50 cases on an MI355X (LSTM_BWD_E); every case prints
    its own figure."""
    name, has_a, b_form, nslab, is_f32, dc_zero, has_cprev = option
    pixels, Hd = shape
    c = lstm_bwd_case(shape, dtype)
    K = U._lib.kernels(dtype)
    numel = pixels * Hd
    g64 = c["gates"].double()
    gi_, gf, gg, go = g64[:, 0], g64[:, 1], g64[:, 2], g64[:, 3]
    cp = c["c_prev"].double() if has_cprev else torch.zeros(pixels, Hd, dtype=torch.float64)
    dh = c["dh_a"].double().clone() if has_a else torch.zeros(pixels, Hd, dtype=torch.float64)
    dhmag = dh.abs()
    stride, dh_b_d, dh_b_before = 0, None, None
    if b_form == "16":
        dh = dh + c["dh_b16"].double()
        dhmag = dhmag + c["dh_b16"].double().abs()
        dh_b_d = dev16(c["dh_b16"], dtype)
    elif b_form == "f32":
        stride = numel + 8 if nslab > 1 else 0                      # slab stride > pixels * Hd_p, a multiple of 4 floats
        buf = torch.full((max(stride, numel) * (nslab - 1) + numel,), GAP)
        for s in range(nslab):
            buf[s * stride: s * stride + numel] = c["slabs"][s].flatten()
            dh = dh + c["slabs"][s].double()
            dhmag = dhmag + c["slabs"][s].double().abs()
        dh_b_before = buf
        dh_b_d = buf.to(DEV)
    dc_in = torch.zeros(pixels, Hd, dtype=torch.float64) if dc_zero else c["dc"].double()
    tc = torch.tanh(c["c_new"].double())
    dct = dc_in + dh * go * (1 - tc * tc)
    ref = torch.stack((dct * gg * gi_ * (1 - gi_), dct * cp * gf * (1 - gf), dct * gi_ * (1 - gg * gg), dh * tc * go * (1 - go)), 1)
    mct = dc_in.abs() + dhmag * go
    mag = torch.stack((mct * gg.abs() * gi_ * (1 - gi_), mct * cp.abs() * gf * (1 - gf), mct * gi_ * (1 + gg * gg), dhmag * go * (1 - go)), 1)
    dc_ref, dc_mag = dct * gf, mct * gf

    # dc_is_zero: dc_io is an output only, so it starts as NaN
    dc_io = nan_like((pixels, Hd), torch.float32) if dc_zero else dev32(c["dc"])
    dgates = nan_like((pixels, 4, Hd), dtype)
    call(K, "uclstm_lstm_bwd_pointwise", ops._p(c["gates_d"]), ops._p(c["c_prev_d"]) if has_cprev else None, ops._p(c["c_new_d"]),
         ops._p(c["dh_a_d"]) if has_a else None, ops._p(dh_b_d), is_f32, nslab, stride, ops._p(dc_io), dc_zero, ops._p(dgates), pixels, Hd)
    what = f"lstm_bwd_pointwise {shape} {name} {tag(dtype)}"
    got_dc = dc_io.cpu().double()
    assert bool(torch.isfinite(got_dc).all()), f"{what}: dc_io not written"
    measured = float(((got_dc - dc_ref).abs() / (dc_mag + 1e-30)).max())
    print(f"[parity] {what}: dc_io max |err| / mag {measured:.3e} (E = {LSTM_BWD_E:.3e})")
    assert measured <= LSTM_BWD_E, f"{what}: dc_io {measured:.3e} x mag > E = {LSTM_BWD_E:.3e}"
    check_elementwise(dgates.float().cpu(), ref, mag, dtype, what + " dgates", f32_units=LSTM_BWD_E)
    if b_form == "f32":
        after = dh_b_d.cpu()
        if is_f32 == 2:                                              # consume-and-clear: slab 0 zeroed, nothing else touched
            assert bool((after[:numel] == 0).all()), f"{what}: slab 0 not cleared"
            assert torch.equal(after[numel:], dh_b_before[numel:]), f"{what}: dh_b changed beyond slab 0"
        else:
            assert torch.equal(after, dh_b_before), f"{what}: dh_b changed"


# ---------------------------------------------------------------------------------------------
# 4. uclstm_lstm_fwd_pointwise_group
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_lstm_fwd_pointwise_group_is_bit_identical_to_single_launches(dtype):
    """Three members that differ in everything the block ranges and the argument table carry: Hd_p 8 / 24 / 64, pixel counts (1, 8 and
    63 blocks), nslab 0 with pre_add / 1 with consume-and-clear / 3 with a slab stride beyond the slab, c_prev and gates_out
    present and NULL."""
    K = U._lib.kernels(dtype)
    L = U._lib
    #          Hd_p pixels nslab clear pre_add c_prev gates
    members = [(8, 37, 0, 0, True, False, True), (24, 300, 1, 1, False, True, False), (64, 1000, 3, 0, True, True, True)]

    def run(grouped):
        torch.manual_seed(42)
        args, keep, out = (L.LstmFwdPwArgs * len(members))(), [], []
        for j, (Hd, pixels, nslab, clear, has_add, has_c, has_g) in enumerate(members):
            N = 64 * ((Hd + 15) // 16)
            slab = pixels * N + 64 if nslab > 1 else 0
            pre = (torch.randn(max(nslab, 1) * (pixels * N + 64)) * 0.7).to(DEV) if nslab else None
            pre0 = None if pre is None else pre.clone()
            add = (torch.randn(pixels, N) * 0.7).to(DEV) if has_add else None
            bias = (torch.randn(N) * 0.3).to(DEV)
            c_prev = torch.randn(pixels, Hd).to(DEV) if has_c else None
            c_out, h_out = nan_like((pixels, Hd), torch.float32), nan_like((pixels, Hd), dtype)
            gates = nan_like((pixels, 4, Hd), dtype) if has_g else None
            keep.append((pre, add, bias, c_prev))
            out.append(dict(c=c_out, h=h_out, g=gates, pre=pre, pre0=pre0, numel=pixels * N))
            if grouped:
                a = args[j]
                a.pre, a.pre_add, a.bias, a.c_prev = (None if t is None else t.data_ptr() for t in (pre, add, bias, c_prev))
                a.c_out, a.h_out, a.gates_out = c_out.data_ptr(), h_out.data_ptr(), None if gates is None else gates.data_ptr()
                a.slab, a.pixels, a.nslab, a.clear, a.Hd_p = slab, pixels, nslab, clear, Hd
            else:
                call(K, "uclstm_lstm_fwd_pointwise", ops._p(pre), nslab, slab, clear, ops._p(add), ops._p(bias), ops._p(c_prev), ops._p(c_out),
                     ops._p(h_out), ops._p(gates), pixels, Hd)
        if grouped:
            call(K, "uclstm_lstm_fwd_pointwise_group", args, len(members))
        torch.cuda.synchronize()
        return out

    single, group = run(False), run(True)
    for j, (s, g) in enumerate(zip(single, group)):
        for k in ("c", "h", "g"):
            if s[k] is None:
                continue
            assert bool(torch.isfinite(s[k].float()).all()), (j, k)
            assert torch.equal(s[k], g[k]), f"member {j} {k}: max diff {float((s[k].float() - g[k].float()).abs().max())}"
    # consume-and-clear zeroes what was read: panel row n = hb*64 + gate*16 + j belongs to hidden channel hb*16 + j, and the rows of
    # the channels beyond Hd_p (24 of the 32 that 128 rows hold) are neither read nor written
    Hd, pixels = members[1][0], members[1][1]
    n = torch.arange(64 * ((Hd + 15) // 16), device=DEV)
    read = ((n // 64) * 16 + n % 16 < Hd)[None, :].expand(pixels, -1).reshape(-1)
    for res in (single, group):
        n1, pre, pre0 = res[1]["numel"], res[1]["pre"], res[1]["pre0"]
        assert bool((pre[:n1][read] == 0).all()), "consumed accumulator not cleared"
        assert torch.equal(pre[:n1][~read], pre0[:n1][~read]) and torch.equal(pre[n1:], pre0[n1:]), "written outside what was read"
        assert torch.equal(res[2]["pre"], res[2]["pre0"]), "three-slab buffer changed"
    print(f"[parity] lstm_fwd_pointwise_group {tag(dtype)}: c_out, h_out, gates_out of 3 members bit-identical to single launches")


# ---------------------------------------------------------------------------------------------
# 5. BatchNorm statistics: uclstm_bn_stats_fwd + uclstm_bn_running_stats, uclstm_bn_finalize, uclstm_bn_bwd_param_grads
# ---------------------------------------------------------------------------------------------
# (groups, tiles per group, Cp, C)
BN_STATS_SHAPES = [
    (3, 1, 8, 5),                 # one tile per group; C < Cp
    (2, 17, 72, 67),              # tiles % 16 != 0; partly filled second 64-channel slab; C < Cp
    (5, 40, 200, 200),            # several groups, C = Cp
]
RTOL = 2.0 ** -21
SENTINEL = 12345.0


def check_rtol(got, ref, what, rtol=RTOL, scale=None):
    got = got.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    e = float(((got - ref).abs() / ((ref.abs() if scale is None else scale) + 1e-300)).max())
    print(f"[parity] {what}: max relative error {e:.2e} (<= {rtol:.2e})")
    assert e <= rtol, f"{what}: {e:.3e} > {rtol:.3e}"
    return e


@pytest.mark.parametrize("momentum_kind", ["momentum 0.1", "cumulative average"])
@pytest.mark.parametrize("shape", BN_STATS_SHAPES, ids=str)
def test_bn_statistics_against_f64(shape, momentum_kind):
    """Both routes (stats_fwd + running_stats, finalize) from the same f32 per-tile (sum, sumsq) partials of data with |mean| / std up
    to 30 (var = E2 - m^2 cancels three digits), against f64 from those partials: var = max(0, E2 - m^2), rstd, scale = gamma*rstd,
    shift = beta - mean*scale; pad channels zero; (mean, variance) left in the tile-0 slots; the running statistics of the
    in-order recursion with momentum 0.1 and with momentum = -(k + 1), k = 4 batches tracked (factor 1 / (k + 1 + g))."""
    groups, tpg, Cp, C = shape
    torch.manual_seed(500 + tpg + Cp)
    per_tile, eps = 24, 1e-5
    count = tpg * per_tile
    std = torch.rand(Cp) + 0.5
    ratio = (torch.rand(Cp) * 29 + 1) * (torch.randint(0, 2, (Cp,)).float() * 2 - 1)      # mean / std, both signs, up to 30
    x = (ratio * std)[None, None, None, :] * (1 + 0.05 * torch.randn(groups, 1, 1, Cp)) + std * torch.randn(groups, tpg, per_tile, Cp)
    x[..., C:] = 0.0
    stats = torch.stack((x.double().sum(2), (x.double() ** 2).sum(2)), -1).float()          # [groups][tpg][Cp][2] f32 partials
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    gamma[::4] *= -1.0
    s64 = stats.double().sum(1)
    m = s64[..., 0] / count
    var = (s64[..., 1] / count - m * m).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    live = (torch.arange(Cp) < C).double()
    g64, b64 = torch.zeros(Cp, dtype=torch.float64), torch.zeros(Cp, dtype=torch.float64)
    g64[:C], b64[:C] = gamma.double(), beta.double()
    want = dict(mean=m * live, rstd=rstd * live, scale=g64 * rstd * live, shift=(b64 - m * g64 * rstd) * live)
    shift_scale = b64.abs() + (m * g64 * rstd).abs()
    # running statistics: same sign as the batch means (the recursion then adds terms of one sign, and a relative bound holds)
    rm0 = torch.full((Cp,), SENTINEL)
    rv0 = torch.full((Cp,), SENTINEL)
    rm0[:C], rv0[:C] = (0.5 * ratio * std)[:C], (torch.rand(C) + 0.5)
    momentum = 0.1 if momentum_kind == "momentum 0.1" else -5.0
    rm, rv = rm0.double().clone(), rv0.double().clone()
    for g in range(groups):
        mom = momentum if momentum >= 0 else 1.0 / (-momentum + g)
        rm = (1 - mom) * rm + mom * m[g]
        rv = (1 - mom) * rv + mom * var[g] * count / (count - 1)
    lib = U._lib.lib

    def outputs():
        return [nan_like((groups, Cp), torch.float32) for _ in range(4)]

    def check_route(route, st, outs, rmd, rvd):
        for k, t in zip(("scale", "shift", "mean", "rstd"), outs):
            got = t.cpu()
            assert bool((got[:, C:] == 0).all()), f"{route} {k}: pad channels not zero"
            if k == "shift":
                check_rtol(got[:, :C], want[k][:, :C], f"bn {route} shift {shape}", scale=shift_scale[:, :C])
            else:
                check_rtol(got[:, :C], want[k][:, :C], f"bn {route} {k} {shape}")
        slot = st.cpu()[:, 0, :C]
        check_rtol(slot[..., 0], m[:, :C], f"bn {route} tile-0 mean {shape}")
        check_rtol(slot[..., 1], var[:, :C], f"bn {route} tile-0 variance {shape}")
        check_rtol(rmd.cpu()[:C], rm[:C], f"bn {route} running_mean {momentum_kind} {shape}", rtol=groups * RTOL)
        check_rtol(rvd.cpu()[:C], rv[:C], f"bn {route} running_var {momentum_kind} {shape}", rtol=groups * RTOL)
        assert bool((rmd.cpu()[C:] == SENTINEL).all()) and bool((rvd.cpu()[C:] == SENTINEL).all()), f"{route}: running statistics written beyond C"

    gd, bd = dev32(gamma), dev32(beta)
    # route 1: one launch for scale / shift / mean / rstd, the momentum steps from what it left in `stats`
    st, outs, rmd, rvd = dev32(stats), outputs(), dev32(rm0), dev32(rv0)
    U._lib.check(lib.uclstm_bn_stats_fwd(ops._p(st), groups, tpg, Cp, C, count, ops._p(gd), ops._p(bd), eps, *[ops._p(t) for t in outs],
                                         ops._stream()), "bn_stats_fwd")
    U._lib.check(lib.uclstm_bn_running_stats(ops._p(st), groups, tpg, Cp, C, count, ops._p(rmd), ops._p(rvd), momentum, ops._stream()),
                 "bn_running_stats")
    check_route("stats_fwd + running_stats", st, outs, rmd, rvd)
    # route 2: uclstm_bn_finalize
    st, outs, rmd, rvd = dev32(stats), outputs(), dev32(rm0), dev32(rv0)
    U._lib.check(lib.uclstm_bn_finalize(ops._p(st), groups, tpg, Cp, C, count, ops._p(gd), ops._p(bd), ops._p(rmd), ops._p(rvd), momentum, eps,
                                        *[ops._p(t) for t in outs], ops._stream()), "bn_finalize")
    check_route("finalize", st, outs, rmd, rvd)
    # evaluation mode (stats == NULL, groups = 1): scale / shift from the running statistics, which stay as they are
    outs = [nan_like((1, Cp), torch.float32) for _ in range(4)]
    U._lib.check(lib.uclstm_bn_finalize(None, 1, 0, Cp, C, 0, ops._p(gd), ops._p(bd), ops._p(rmd), ops._p(rvd), momentum, eps,
                                        *[ops._p(t) for t in outs], ops._stream()), "bn_finalize (evaluation)")
    rm32, rv32 = rmd.cpu().double()[:C], rvd.cpu().double()[:C]
    ers = 1.0 / torch.sqrt(rv32 + eps)
    ew = dict(scale=gamma.double() * ers, shift=beta.double() - rm32 * gamma.double() * ers, mean=rm32, rstd=ers)
    for k, t in zip(("scale", "shift", "mean", "rstd"), outs):
        got = t.cpu()[0]
        assert bool((got[C:] == 0).all()), f"evaluation {k}: pad channels not zero"
        check_rtol(got[:C], ew[k], f"bn finalize evaluation {k} {shape}",
                   scale=(beta.double().abs() + (rm32 * gamma.double() * ers).abs()) if k == "shift" else None)
    assert torch.equal(rmd.cpu()[:C].double(), rm32) and bool((rmd.cpu()[C:] == SENTINEL).all()) and torch.equal(rvd.cpu()[:C].double(), rv32)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", BN_STATS_SHAPES, ids=str)
def test_bn_bwd_param_grads_against_f64(shape, accumulate):
    """dbeta[c] = (accumulate ? dbeta[c] : 0) + sum_g sums[g][c][0], dgamma likewise from sums[g][c][1], c < C; nothing beyond C."""
    groups, tpg, Cp, C = shape
    torch.manual_seed(600 + Cp)
    sums = torch.randn(groups, Cp, 2)
    prior = torch.randn(2, Cp)
    prior[:, C:] = SENTINEL
    dgamma, dbeta = dev32(prior[0]), dev32(prior[1])
    U._lib.check(U._lib.lib.uclstm_bn_bwd_param_grads(ops._p(dev32(sums)), groups, Cp, C, ops._p(dgamma), ops._p(dbeta), accumulate, ops._stream()),
                 "bn_bwd_param_grads")
    for name, got, j, p in (("dbeta", dbeta.cpu(), 0, prior[1]), ("dgamma", dgamma.cpu(), 1, prior[0])):
        ref = sums[:, :C, j].double().sum(0) + (p[:C].double() if accumulate else 0.0)
        terms = sums[:, :C, j].double().abs().sum(0) + (p[:C].double().abs() if accumulate else 0.0)
        check_sums(got[:C], ref, terms, f"bn_bwd_param_grads {name} {shape} accumulate={accumulate}")
        assert bool((got[C:] == SENTINEL).all()), f"{name} written beyond C"
