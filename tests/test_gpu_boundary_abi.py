"""The kernels at the boundary of a module -- layout converters, first-layer im2col, stand-alone MaxPool2d(2), the OutConv 1x1 head,
SpatialAttention and the loss gradient -- each called directly at the C ABI (bf16 and fp16 wherever the entry point has a twin)
and compared with the f64 references of tests/boundary_cases.py, which restate include/uclstm.h and are pinned to PyTorch's own
f64 code in tests/test_cabi_and_host.py.

The module tests reach these kernels through ops.* at one or two friendly shapes with rel-L2 tolerances; one misrouted arg-max
gradient, a lane reduction of the wrong width or a mask read one element off does not move a rel-L2.  The case tables hold the
smallest shapes that reach every path: every instance of the OutConv lane kernel and the generic one at 1 / 3 / 25 / 64 chunks,
both rounds of the attention channel loop, more than one block and more than one trip of every grid-stride loop (item counts
asserted against the launch caps in boundary_cases.py), H = 1, W = 1, odd sizes, tap boundaries inside a 16-byte chunk, all 15
tie patterns of a pooling window, arg-max ties inside a chunk, across lanes and across rounds.

Bounds (helpers and constants of tests/test_gpu_pointwise_abi.py; outputs are pre-filled with NaN or a sentinel, no element is
left out):
  * layout, im2col, MaxPool forward, MaxPool backward without `add`: bit-exact against x.to(dtype) of the f64 reference (round to
    nearest even; inputs hold signed zeros, infinities, exact half-way points of both parities, 65520 and 16-bit subnormals);
    16-bit -> f32 is the stored value, bit for bit; pad channels / pad taps exactly zero
  * MaxPool backward with `add`, OutConv da, attention out / dx: check_elementwise, half a 16-bit unit + 2^-21 * sum|terms|
  * arg-max: the reference's first maximal channel at every pixel; desc max: exact
  * OutConv y, attention desc mean / dpre / ddesc: |err| <= (n + 2) * 2^-24 * sum|terms|, n = the longest chain of f32 additions the
    case reaches (y: C + 1 generic, 8 + log2(LPP) + 1 lanes; mean: 8 per round of the channel loop + 6 shuffle steps; dpre: the same
    + 2 for the two factors; ddesc: k * k)
  * OutConv dw / db: (2e-6 + nblocks * 2^-24) * sum|terms| (f32 atomics, one rounding per block)
  * attention att: |err| <= 0.25 * (2 k^2 + 2) * 2^-24 * sum|conv terms| + ATT_EXPF_ALLOWANCE against sigmoid in f64 of the
    convolution of the kernel's own desc (0.25 = the largest slope of the sigmoid).  The allowance covers __expf, whose error is not
    specified: 4 x the worst |err| beyond the first term measured on MI355X over all cases, not below 2^-22.  Measured: worst |err|
    1.35e-7 (0.146 of the whole bound), and at no pixel does |err| exceed the first term (worst |err| - term = -2.9e-8), so the
    allowance is its floor, 2^-22 = 2.4e-7 -- far below the 1e-5 that the condition on it allows (att lies in (0, 1))
  * attention dw: check_sums at 2e-6 against the f64 sum of the kernel's own dpre x desc
  * loss gradient: |err| <= 8 * 2^-24 * (|c1| w m + |c2| sum|gradient terms|): fewer than eight f32 roundings; the signs and the
    mask sums are exact on the 1/64 input grid

fp16 runs the backward kernels on gradients x 1024, as fp16 training does.
"""
import math

import pytest
import torch

import boundary_cases as BC
from test_gpu_pointwise_abi import (DEV, DTYPES, call, check_elementwise, check_sums, dev16, dev32, loss_scale, nan_like, r16, tag)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

ATT_EXPF_ALLOWANCE = 2.0 ** -22        # the floor: measured on MI355X, |err| never exceeds the convolution term (worst |err| 1.35e-7)
assert ATT_EXPF_ALLOWANCE <= 1e-5
SENTINEL = 0x5A5A                      # 16-bit pattern of elements the kernel must not write
F32_UNIT = 2.0 ** -24


def p_(t):
    return ops._p(t)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def nan32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def assert_bits(got, ref, what):
    """got == ref bit for bit (signed zeros, infinities and subnormals included); ref holds no NaN, so neither may got."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = bits(got) != bits(ref)
    n = int(bad.sum())
    print(f"[parity] {what}: {'bit-exact' if n == 0 else f'{n} elements differ'} over {bad.numel()} elements")
    if n:
        i = int(bad.flatten().nonzero()[0])
        g, r = got.detach().cpu().flatten()[i], ref.flatten()[i]
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ; first at flat index {i}: got {float(g)!r}, want {float(r)!r}")


def check_f32(got, ref, bound, what):
    """|got - ref| <= bound at every element of an f32 output (got finite everywhere)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: elements not written"
    d = (got - ref).abs()
    worst = float((d / (bound + 1e-300)).max())
    print(f"[parity] {what}: worst |err| / bound {worst:.3f} (<= 1), max |err| {float(d.max()):.3e} over {d.numel()} elements")
    bad = int((d > bound).sum())
    assert bad == 0, f"{what}: {bad} of {d.numel()} elements beyond the bound (worst {worst:.3f} x)"
    return worst


def K_(dtype):
    return U._lib.kernels(dtype)


# ---------------------------------------------------------------------------------------------
# 1. layout converters and the first-layer im2col: bit-exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.LAYOUT_CASES, ids=str)
def test_nchw_to_nhwc_and_back_bit_exact(case, dtype):
    """uclstm_nchw_to_nhwc (plain and time-major), uclstm_nchw_grad_to_nhwc and uclstm_nhwc_to_nchw."""
    n_img, C, Cp, H, W, inner = case
    K = K_(dtype)
    x = BC.layout_input(case, dtype)
    xd = dev32(x)
    out = nan_like((n_img, H, W, Cp), dtype)
    call(K, "uclstm_nchw_to_nhwc", p_(xd), p_(out), n_img, C, Cp, H, W, *BC.layout_strides(case))
    ref = BC.nchw_to_nhwc_ref(x.double(), Cp, inner).to(dtype)
    assert_bits(out, ref, f"nchw_to_nhwc {case} {tag(dtype)}")
    assert bool((bits(out)[..., C:] == 0).all()), "pad channels are not +0"
    out = nan_like((n_img, H, W, Cp), dtype)
    call(K, "uclstm_nchw_grad_to_nhwc", p_(xd), p_(out), n_img, C, Cp, H, W)
    assert_bits(out, BC.nchw_to_nhwc_ref(x.double(), Cp, 1).to(dtype), f"nchw_grad_to_nhwc {case} {tag(dtype)}")
    a = BC.stored16_input((n_img, H, W, Cp), dtype)
    back = nan32(n_img, C, H, W)
    ad = a.to(DEV)
    call(K, "uclstm_nhwc_to_nchw", p_(ad), p_(back), n_img, C, Cp, H, W)
    assert_bits(back, BC.nhwc_to_nchw_ref(a.double(), C).float(), f"nhwc_to_nchw {case} {tag(dtype)}")


@pytest.mark.parametrize("case", BC.LAYOUT_F32_CASES, ids=str)
def test_f32_layout_pair_bit_exact(case):
    """uclstm_nchw_to_nhwc_f32 / uclstm_nhwc_to_nchw_f32 (cell state; one symbol for both activation types)."""
    n_img, C, Cp, H, W = case
    BC.manual_seed(9, *case)
    x = BC.plant(torch.randn(n_img, C, H, W), BC.layout_specials(torch.bfloat16))
    xd, out = dev32(x), nan32(n_img, H, W, Cp)
    call(U._lib.lib, "uclstm_nchw_to_nhwc_f32", p_(xd), p_(out), n_img, C, Cp, H, W)
    assert_bits(out, BC.nchw_to_nhwc_ref(x, Cp), f"nchw_to_nhwc_f32 {case}")
    a = BC.plant(torch.randn(n_img, H, W, Cp), BC.layout_specials(torch.float16))        # pad channels hold data: they must not leak
    ad, back = dev32(a), nan32(n_img, C, H, W)
    call(U._lib.lib, "uclstm_nhwc_to_nchw_f32", p_(ad), p_(back), n_img, C, Cp, H, W)
    assert_bits(back, BC.nhwc_to_nchw_ref(a, C), f"nhwc_to_nchw_f32 {case}")


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.IM2COL_CASES, ids=str)
def test_im2col3x3_first_bit_exact(case, dtype):
    """uclstm_im2col3x3_first: element 0 of every image -- the address the kernel clamps an outside tap to -- holds inf, so a tap
    that is masked by anything but a select shows as NaN."""
    n_img, C, Kp, H, W, inner = case
    BC.manual_seed(7, *case)
    x = torch.randn(n_img, C, H, W)
    x[:, 0, 0, 0] = math.inf
    xd, out = dev32(x), nan_like((n_img, H, W, Kp), dtype)
    call(K_(dtype), "uclstm_im2col3x3_first", p_(xd), p_(out), n_img, C, Kp, H, W, *BC.layout_strides(case))
    assert_bits(out, BC.im2col_ref(x.double(), Kp, inner).to(dtype), f"im2col3x3_first {case} {tag(dtype)}")
    assert bool((bits(out)[..., 9 * C:] == 0).all()), "pad taps are not +0"


# ---------------------------------------------------------------------------------------------
# 2. MaxPool2d(2)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.MAXPOOL_CASES, ids=str)
def test_maxpool2_fwd_bwd_against_f64(case, dtype):
    """Forward: the window maximum, exactly.  Backward without `add`: dp at the first maximum in scan order and +0 elsewhere, bit
    for bit, for all 15 sets of tied positions; with odd H / W the trailing row / column keeps the sentinel it was filled with.
    Backward with `add` (even shapes): add + scatter(dp) within half a unit."""
    n_img, H, W, Cp = case
    K, S = K_(dtype), loss_scale(dtype)
    Ho, Wo = H // 2, W // 2
    a = BC.maxpool_input(case, dtype)
    ad = dev16(a, dtype)
    p = nan_like((n_img, Ho, Wo, Cp), dtype)
    call(K, "uclstm_maxpool2_fwd", p_(ad), p_(p), n_img, H, W, Cp)
    ref_p, best = BC.maxpool_ref(a.double())
    assert bool((ref_p != 0).all())
    assert_bits(p, ref_p.to(dtype), f"maxpool2_fwd {case} {tag(dtype)}")
    BC.manual_seed(10, *case)
    dp = r16(S * (torch.randn(n_img, Ho, Wo, Cp) + 1.0), dtype)
    dp = torch.where(dp == 0, torch.ones_like(dp), dp)
    dpd = dev16(dp, dtype)
    da = torch.full((n_img, H, W, Cp), SENTINEL, dtype=torch.int16, device=DEV).view(dtype)
    call(K, "uclstm_maxpool2_bwd", p_(ad), p_(dpd), None, p_(da), n_img, H, W, Cp)
    ref, written = BC.maxpool_bwd_ref(a.double(), dp.double())
    got_bits = bits(da)
    assert bool((got_bits[~written] == SENTINEL).all()), "the kernel wrote pixels that no window covers"
    assert int((~written).sum()) == n_img * (H * W - 4 * Ho * Wo)
    want = torch.where(written[..., None], bits(ref.to(dtype)), torch.full_like(got_bits, SENTINEL))
    assert_bits(da, want.view(dtype), f"maxpool2_bwd {case} {tag(dtype)}")
    tied = int(((BC.windows(a) == ref_p).sum(0) >= 2).sum())
    print(f"[parity] maxpool2_bwd {case} {tag(dtype)}: {tied} of {best.numel()} window channels hold a tie")
    if case in BC.MAXPOOL_ADD_CASES:
        add = r16(S * (torch.randn(n_img, H, W, Cp) + 1.0), dtype)
        addd, da = dev16(add, dtype), nan_like((n_img, H, W, Cp), dtype)
        call(K, "uclstm_maxpool2_bwd", p_(ad), p_(dpd), p_(addd), p_(da), n_img, H, W, Cp)
        ref2, _ = BC.maxpool_bwd_ref(a.double(), dp.double(), add.double())
        check_elementwise(da.float().cpu(), ref2, add.double().abs() + ref.abs(), dtype, f"maxpool2_bwd + add {case} {tag(dtype)}")


# ---------------------------------------------------------------------------------------------
# 3. OutConv 1x1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.OUTCONV_FWD_CASES, ids=str)
def test_outconv_fwd_against_f64(case, dtype):
    n_img, HW, C, Cp, Co, bias = case
    a, w, b, _ = BC.outconv_operands(case, dtype)
    ad, wd, bd, y = dev16(a, dtype), dev32(w), dev32(b), nan32(n_img, Co, HW)
    call(K_(dtype), "uclstm_outconv_fwd", p_(ad), p_(wd), p_(bd) if bias else None, p_(y), n_img, HW, Cp, C, Co)
    ref, mag = BC.outconv_fwd_ref(a, w, b if bias else None, n_img, HW)
    n = BC.outconv_fwd_chain(C, Cp)
    kernel = f"lanes<{BC.outconv_lanes(Cp)}>" if BC.outconv_lanes(Cp) else f"generic, {Cp // 8} chunks"
    check_f32(y, ref, (n + 2) * F32_UNIT * mag, f"outconv_fwd y {case} {tag(dtype)} ({kernel}, n = {n})")


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.OUTCONV_DA_CASES, ids=str)
def test_outconv_bwd_da_against_f64(case, dtype):
    """da = act16(sum_co dy * w) within half a unit, pad channels exactly zero -- also at the pixel whose dy is inf, where the valid
    channels must be the infinities of the sign of w."""
    n_img, HW, C, Cp, Co, with_inf = case
    a, w, _, dy = BC.outconv_operands(case, dtype, loss_scale(dtype))
    inf_pix = 1 * HW + 3
    if with_inf:
        dy[1, 0, 3] = math.inf
    ad, wd, dyd, da = dev16(a, dtype), dev32(w), dev32(dy), nan_like((n_img * HW, Cp), dtype)
    call(K_(dtype), "uclstm_outconv_bwd", p_(ad), p_(wd), p_(dyd), p_(da), None, None, n_img, HW, Cp, C, Co)
    got = da.float().cpu()
    assert bool((bits(da)[:, C:] == 0).all()), "pad channels are not +0"
    if with_inf:
        assert torch.equal(got[inf_pix, :C], torch.sign(w[0]) * math.inf) and bool((w[0] != 0).all())
        dy[1, 0, 3] = 0.0
        got[inf_pix] = 0.0
    ref, mag = BC.outconv_bwd_ref(a, w, dy, Cp)[:2]
    if with_inf:
        ref[inf_pix], mag[inf_pix] = 0.0, 0.0
    check_elementwise(got, ref, mag, dtype, f"outconv_bwd da {case} {tag(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.OUTCONV_DW_CASES, ids=str)
def test_outconv_bwd_dw_db_against_f64(case, dtype):
    """dw / db accumulated with f32 atomics onto zeroed buffers; with exactly one of them NULL no parameter-gradient kernel runs
    and the other buffer keeps its NaN fill (include/uclstm.h)."""
    n_img, HW, C, Cp, Co = case
    K = K_(dtype)
    a, w, _, dy = BC.outconv_operands(case, dtype, loss_scale(dtype))
    ad, wd, dyd = dev16(a, dtype), dev32(w), dev32(dy)
    dw, db = torch.zeros(Co, C, device=DEV), torch.zeros(Co, device=DEV)
    call(K, "uclstm_outconv_bwd", p_(ad), p_(wd), p_(dyd), None, p_(dw), p_(db), n_img, HW, Cp, C, Co)
    _, _, ref_w, terms_w, ref_b, terms_b = BC.outconv_bwd_ref(a, w, dy, Cp)
    nblocks = BC.outconv_dw_blocks(n_img * HW)
    tol = 2e-6 + nblocks * F32_UNIT
    check_sums(dw.cpu(), ref_w, terms_w, f"outconv_bwd dw {case} {tag(dtype)} ({nblocks} blocks)", tol=tol)
    check_sums(db.cpu(), ref_b, terms_b, f"outconv_bwd db {case} {tag(dtype)} ({nblocks} blocks)", tol=tol)
    dw, db = nan32(Co, C), nan32(Co)
    call(K, "uclstm_outconv_bwd", p_(ad), p_(wd), p_(dyd), None, p_(dw), None, n_img, HW, Cp, C, Co)
    call(K, "uclstm_outconv_bwd", p_(ad), p_(wd), p_(dyd), None, None, p_(db), n_img, HW, Cp, C, Co)
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()), "a parameter-gradient kernel ran with dw or db NULL"


# ---------------------------------------------------------------------------------------------
# 4. SpatialAttention
# ---------------------------------------------------------------------------------------------
def attn_forward(case, dtype):
    n_img, H, W, C, Cp, k = case
    pixels = n_img * H * W
    x, planted = BC.attn_input(case, dtype)
    w = BC.attn_weight(case)
    xd, wd = dev16(x, dtype), dev32(w)
    out, att, desc = nan_like((n_img, H, W, Cp), dtype), nan32(n_img, H, W), nan32(n_img, H, W, 2)
    arg = torch.full((n_img, H, W), -7, dtype=torch.int32, device=DEV)
    call(K_(dtype), "uclstm_attention_fwd", p_(xd), p_(wd), p_(out), p_(att), p_(desc), p_(arg), n_img, H, W, Cp, C, k)
    return dict(x=x, w=w, xd=xd, wd=wd, out=out, att=att, desc=desc, arg=arg, pixels=pixels, planted=planted)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.ATTN_CASES, ids=str)
def test_attention_fwd_against_f64(case, dtype):
    n_img, H, W, C, Cp, k = case
    f = attn_forward(case, dtype)
    what = f"{case} {tag(dtype)}"
    mean, mx, first, absmean = BC.attn_desc_ref(f["x"], C)
    arg = f["arg"].cpu().long()
    wrong = int((arg != first).sum())
    print(f"[parity] attention arg-max {what}: {wrong} of {arg.numel()} pixels differ from the first maximal channel; "
          f"{int(((f['x'].double()[..., :C] == mx[..., None]).sum(-1) >= 2).sum())} pixels hold a tie, planted: "
          f"{sorted(kind for kind, _ in f['planted'].values())}")
    assert wrong == 0, f"attention arg-max {what}: {wrong} pixels are not routed to the first maximal channel"
    desc = f["desc"].cpu()
    assert torch.equal(desc[..., 1].double(), mx), "desc max is not the maximum over the valid channels"
    n = 8 * BC.attn_rounds(Cp) + 6
    check_f32(desc[..., 0], mean, (n + 2) * F32_UNIT * absmean, f"attention desc mean {what} (n = {n})")
    pre, mag = BC.attn_conv(desc.double(), f["w"])
    ref_att = 1.0 / (1.0 + torch.exp(-pre))
    assert float(ref_att.min()) > 2.0 ** -10                     # x * att stays a normal fp16 number (|x| >= 0.25)
    conv_term = 0.25 * (2 * k * k + 2) * F32_UNIT * mag
    att = f["att"].cpu()
    assert bool(torch.isfinite(att).all())
    beyond = float(((att.double() - ref_att).abs() - conv_term).max())
    print(f"[parity] attention att {what}: worst |err| beyond the convolution term {beyond:.3e} (allowance {ATT_EXPF_ALLOWANCE:.3e})")
    check_f32(att, ref_att, conv_term + ATT_EXPF_ALLOWANCE, f"attention att {what}")
    ref_out = f["x"].double() * att.double()[..., None]
    check_elementwise(f["out"].float().cpu(), ref_out, ref_out.abs(), dtype, f"attention out {what}")
    assert bool((bits(f["out"])[..., C:] == 0).all()), "pad channels are not +0"


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", BC.ATTN_CASES, ids=str)
def test_attention_bwd_against_f64(case, dtype):
    """dpre, ddesc (read back from `scratch`), dw (dw_accumulate 0 and 1, NULL) and dx.  Each stage is compared with f64 on the
    kernel's own inputs of that stage: att / desc / arg-max from the forward launch (checked on their own above), dpre for ddesc
    and dw, ddesc for dx."""
    n_img, H, W, C, Cp, k = case
    f = attn_forward(case, dtype)
    K, S, pixels = K_(dtype), loss_scale(dtype), f["pixels"]
    what = f"{case} {tag(dtype)}"
    BC.manual_seed(11, *case)
    dout = r16(S * torch.randn(n_img, H, W, Cp), dtype)          # pad channels hold data: dx must be zero there all the same
    doutd = dev16(dout, dtype)
    args = (p_(f["xd"]), p_(doutd), p_(f["wd"]), p_(f["att"]), p_(f["desc"]), p_(f["arg"]))
    geom = (n_img, H, W, Cp, C, k)
    scratch, dx, dw = nan32(3 * pixels + 2), nan_like((n_img, H, W, Cp), dtype), nan32(2, k, k)
    call(K, "uclstm_attention_bwd", *args, p_(dx), p_(dw), 0, p_(scratch), *geom)
    x64, d64 = f["x"].double(), dout.double()
    att, desc, arg = f["att"].cpu().double(), f["desc"].cpu().double(), f["arg"].cpu().long()
    sc = scratch.cpu()
    off = (pixels + 1) & ~1
    dpre, ddesc = sc[:pixels].view(n_img, H, W), sc[off:off + 2 * pixels].view(n_img, H, W, 2)
    # dpre = (sum_c dout * x) * att * (1 - att)
    slope = att * (1.0 - att)
    n = 8 * BC.attn_rounds(Cp) + 6 + 2
    check_f32(dpre, (x64 * d64).sum(-1) * slope, (n + 2) * F32_UNIT * (x64 * d64).abs().sum(-1) * slope, f"attention dpre {what} (n = {n})")
    ref_dd, mag_dd = BC.attn_conv(dpre.double(), f["w"], transpose=True)
    check_f32(ddesc, ref_dd, (k * k + 2) * F32_UNIT * mag_dd, f"attention ddesc {what}")
    ref_dw, terms = BC.attn_dw_ref(dpre.double(), desc, k)
    check_sums(dw.cpu(), ref_dw, terms, f"attention dw {what}")
    pre_dw = torch.randn(2, k, k) * float(ref_dw.abs().max() + 1.0)
    dw1, dx1, scratch1 = dev32(pre_dw.clone()), nan_like((n_img, H, W, Cp), dtype), nan32(3 * pixels + 2)
    call(K, "uclstm_attention_bwd", *args, p_(dx1), p_(dw1), 1, p_(scratch1), *geom)
    check_sums(dw1.cpu(), pre_dw.double() + ref_dw, pre_dw.double().abs() + terms, f"attention dw accumulate {what}")
    keep, dx2, scratch2 = nan32(2, k, k), nan_like((n_img, H, W, Cp), dtype), nan32(3 * pixels + 2)
    call(K, "uclstm_attention_bwd", *args, p_(dx2), None, 0, p_(scratch2), *geom)
    assert bool(torch.isnan(keep).all()) and torch.equal(bits(dx2), bits(dx)) and torch.equal(bits(dx1), bits(dx))
    # dx = dout * att + ddesc[0] / C + (c == arg) * ddesc[1]
    dd = ddesc.double()
    onehot = (torch.arange(Cp) == arg[..., None]).double()
    ref_dx = d64 * att[..., None] + dd[..., 0:1] / C + onehot * dd[..., 1:2]
    mag_dx = (d64 * att[..., None]).abs() + dd[..., 0:1].abs() / C + onehot * dd[..., 1:2].abs()
    ref_dx[..., C:], mag_dx[..., C:] = 0.0, 0.0
    check_elementwise(dx.float().cpu(), ref_dx, mag_dx, dtype, f"attention dx {what}")
    assert bool((bits(dx)[..., C:] == 0).all()), "pad channels are not +0"


# ---------------------------------------------------------------------------------------------
# 5. loss gradient
# ---------------------------------------------------------------------------------------------
LOSS_RUNS = [(c, m, BC.LOSS_COEFS) for c in BC.LOSS_BWD_CASES for m in (False, True)] + [((5, 17, 19), True, (0.37, 0.0))]


@pytest.mark.parametrize("case,masked,coefs", LOSS_RUNS, ids=str)
def test_loss_bwd_against_f64(case, masked, coefs):
    planes, H, W = case
    yp, y, mask = BC.loss_input(case, masked)
    cd = torch.tensor(coefs, dtype=torch.float32, device=DEV)
    ypd, yd, md, grad = dev32(yp), dev32(y), dev32(mask) if masked else None, nan32(planes, H, W)
    call(U._lib.lib, "uclstm_loss_bwd", p_(ypd), p_(yd), p_(md), p_(cd), p_(grad), planes, H, W)
    c1, c2 = (float(v) for v in cd.cpu().double())
    ref, mag = BC.loss_bwd_ref(yp, y, mask, c1, c2)
    check_f32(grad, ref, 8 * F32_UNIT * mag, f"loss_bwd {case} {'masked' if masked else 'mask NULL'} coefs {coefs}")
