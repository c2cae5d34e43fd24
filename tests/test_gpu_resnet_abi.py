"""The kernels of csrc/resnet.hip called directly at the C ABI, in bf16 and fp16, every element compared with f64 computed from the
device's own stored inputs (tests/resnet_cases.py), and the stride-2 descriptors of the implicit-GEMM forward family
(3x3 / scale 2 / pad 1 and 1x1 / scale 2 / pad 0: the ResNet encoder's downsampling layers) with the forward family's own
reference, runner and bounds (tests/igemm_cases.py, tests/test_gpu_igemm_abi.py).

Bounds are counted, none is fitted (u = 2^-24; u16 = 2^-8 bf16 / 2^-11 fp16, one rounding to the storage type):
  * im2col7x7s2_first, maxpool3s2_fwd, upsample2_fwd    bit-exact (a gather, a selection, a copy; the gather rounds f32 -> 16 bit once)
  * upsample2_bwd                                       u16 |ref| + 3 u sum|terms|            (three f32 additions)
  * bn_add_relu                                         u16 |ref| + 5 u sum|terms|            (two products, three additions; ReLU is 1-Lipschitz)
  * head3x3_fwd (f32 output)                            (9 C + 1) u sum|terms|               (9 C products accumulated onto the bias)
  * head3x3_bwd da                                      u16 |ref| + 9 Co u sum|terms|
  * head3x3_bwd dw, db (f32, += onto a preload)         (pixels + 2) u sum|terms|            (no summation order passes an element through
                                                        more additions than there are pixels; + the product, + the add onto the preload)
  * head3x3_bwd_ordered                                 the same bound; bit-identical between two calls and to the sum of its own
                                                        partial rows taken in row order on the host in f32
Every output sits between guard zones of a NaN pattern and starts out filled with it; no element is excluded.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import igemm_cases as IC
import resnet_cases as RC
import test_gpu_igemm_abi as T
from test_gpu_igemm_abi import Guarded, check_16bit, dev32, tag

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_convlstm_amd import ops

L = IC.L
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
N_IMG = 3
SIZES = [(5, 6), (8, 8), (16, 12)]
CPS = [8, 72]
U32 = RC.U32


def stream():
    return ops._stream()


def rand16(shape, dtype, seed, scale=0.8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def put(x):
    """A host tensor on the device inside guard zones (inputs are guarded too: an aligned body, and nothing valid next to it)."""
    b = Guarded(x.shape, x.dtype)
    b.load(x)
    return b


def call(fn, what, *args):
    L.check(fn(*args, stream()), what)
    torch.cuda.synchronize()


def assert_bits(buf, ref, what):
    got, untouched = buf.read()
    assert not bool(untouched.any()), f"{what}: {int(untouched.sum())} elements not written"
    assert torch.equal(got, ref.double()), f"{what}: {int((got != ref.double()).sum())} of {got.numel()} elements differ"


def assert_within(buf, ref, bound, what, dtype):
    got, untouched = buf.read()
    assert not bool(untouched.any()), f"{what}: {int(untouched.sum())} elements not written"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    d = (got - ref).abs()
    worst = float((d / (bound + 1e-30)).max())
    print(f"[parity] {what} {tag(dtype)}: worst |err| / bound {worst:.3f} (<= 1), max |err| {float(d.max()):.3e} over {d.numel()} elements")
    T.note(what.split(" ")[0], dtype, worst)
    assert int((d > bound + 1e-30).sum()) == 0, f"{what}: {int((d > bound + 1e-30).sum())} elements beyond the bound (worst {worst:.3f} x)"
    return got


# ---------------------------------------------------------------------------------------------
# bit-exact kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("bt", [(3, 1), (3, 2)], ids=lambda v: f"B{v[0]}T{v[1]}")
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_im2col7x7s2_first_is_the_gather(hw, bt, dtype):
    (H, W), (B, Tn), Cc = hw, bt, 2
    x = torch.randn(B, Tn, Cc, H, W, generator=torch.Generator().manual_seed(H * W + Tn))
    Kp = (49 * Cc + 7) // 8 * 8
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = Guarded((B * Tn, Ho, Wo, Kp), dtype)
    xd = dev32(x)
    call(L.kernels(dtype).uclstm_im2col7x7s2_first, "im2col7x7s2_first", xd.data_ptr(), out.ptr(), B * Tn, Cc, Kp, H, W, B, Cc * H * W,
         Tn * Cc * H * W)
    ref = RC.im2col7_ref(x, B, Tn, Kp).to(dtype)
    assert float((ref[..., :49 * Cc] != 0).float().mean()) > 0.3 and bool((ref[..., 49 * Cc:] == 0).all())
    assert_bits(out, ref, "im2col7x7s2_first")
    # through the host wrapper (the model's own call)
    with ops.compute_dtype(dtype):
        from unet_convlstm_amd import resnet as R
        assert torch.equal(R.im2col7x7s2_first(xd).cpu().double(), ref.double())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("Cp", CPS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_maxpool3s2_and_upsample2_forward_are_bit_exact(hw, Cp, dtype):
    H, W = hw
    a = rand16((N_IMG, H, W, Cp), dtype, H + Cp)          # negative values too: a zero padding would win over them
    ad = put(a)
    K = L.kernels(dtype)
    p = Guarded((N_IMG, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cp), dtype)
    call(K.uclstm_maxpool3s2_fwd, "maxpool3s2_fwd", ad.ptr(), p.ptr(), N_IMG, H, W, Cp)
    ref = RC.maxpool3s2_ref(a)
    assert float((ref < 0).double().mean()) > 0.001
    assert_bits(p, ref, "maxpool3s2_fwd")
    up = Guarded((N_IMG, 2 * H, 2 * W, Cp), dtype)
    call(K.uclstm_upsample2_fwd, "upsample2_fwd", ad.ptr(), up.ptr(), N_IMG, H, W, Cp)
    assert_bits(up, RC.upsample2_ref(a), "upsample2_fwd")


# ---------------------------------------------------------------------------------------------
# one 16-bit rounding of an f32 expression
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("Cp", CPS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_upsample2_bwd_against_f64(hw, Cp, dtype):
    H, W = hw
    d = rand16((N_IMG, 2 * H, 2 * W, Cp), dtype, 3 * H + Cp)
    dd, da = put(d), Guarded((N_IMG, H, W, Cp), dtype)
    call(L.kernels(dtype).uclstm_upsample2_bwd, "upsample2_bwd", dd.ptr(), da.ptr(), N_IMG, H, W, Cp)
    ref, mag = RC.upsample2_bwd_ref(d)
    assert_within(da, ref, RC.round16_bound(ref, mag, dtype, 3), "upsample2_bwd", dtype)
    da2 = Guarded((N_IMG, H, W, Cp), dtype)
    call(L.kernels(dtype).uclstm_upsample2_bwd, "upsample2_bwd", dd.ptr(), da2.ptr(), N_IMG, H, W, Cp)
    assert torch.equal(da.read()[0], da2.read()[0])          # a pure function of its input


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("pairs", ["both", "z", "none"])
@pytest.mark.parametrize("Cp", CPS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_bn_add_relu_against_f64(hw, Cp, pairs, dtype):
    H, W = hw
    pixels = N_IMG * H * W
    z, r = rand16((pixels, Cp), dtype, H + Cp + 1), rand16((pixels, Cp), dtype, H + Cp + 2)
    g = torch.Generator().manual_seed(Cp + H)
    vec = lambda signed: ((torch.rand(Cp, generator=g) + 0.5) * (torch.where(torch.arange(Cp) % 3 == 0, -1.0, 1.0) if signed else 1.0))
    sc, sh, rs, rh = vec(True), torch.randn(Cp, generator=g) * 0.5, vec(True), torch.randn(Cp, generator=g) * 0.5
    if pairs != "both":
        rs = rh = None
    if pairs == "none":
        sc = sh = None
    keep = [None if t is None else dev32(t) for t in (sc, sh, rs, rh)]
    ptr = [None if t is None else t.data_ptr() for t in keep]
    zd, rd, a = put(z), put(r), Guarded((pixels, Cp), dtype)
    call(L.kernels(dtype).uclstm_bn_add_relu, "bn_add_relu", zd.ptr(), ptr[0], ptr[1], rd.ptr(), ptr[2], ptr[3], a.ptr(), pixels, Cp)
    ref, mag = RC.bn_add_relu_ref(z, sc, sh, r, rs, rh)
    assert 0.2 < float((ref > 0).double().mean()) < 0.8
    assert_within(a, ref, RC.round16_bound(ref, mag, dtype, 5), f"bn_add_relu {pairs}", dtype)


# ---------------------------------------------------------------------------------------------
# the 3x3 head
# ---------------------------------------------------------------------------------------------
HEAD_SIZES = SIZES + [(40, 36)]          # 4320 pixels: three pixel ranges of the parameter-gradient reduction (one up to 2048)


def head_case(hw, C, Co, dtype):
    H, W = hw
    Cp = (C + 7) // 8 * 8
    g = torch.Generator().manual_seed(H * W + C + Co)
    a = rand16((N_IMG, H, W, Cp), dtype, H + C)
    a[..., C:] = 0
    w = torch.randn(Co, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.3
    dy = torch.randn(N_IMG, Co, H, W, generator=g)
    return H, W, Cp, a, w, b, dy


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("Co", [1, 3])
@pytest.mark.parametrize("C", [16, 10])
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_head3x3_fwd_against_f64(hw, C, Co, dtype):
    H, W, Cp, a, w, b, _ = head_case(hw, C, Co, dtype)
    ad, wd, bd = put(a), dev32(w), dev32(b)
    y = Guarded((N_IMG, Co, H, W), torch.float32)
    call(L.kernels(dtype).uclstm_head3x3_fwd, "head3x3_fwd", ad.ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr(), N_IMG, H, W, Cp, C, Co)
    ref, mag = RC.head_fwd_ref(a, w, b, C)
    assert_within(y, ref, (9 * C + 1) * U32 * mag, "head3x3_fwd", dtype)
    y0 = Guarded((N_IMG, Co, H, W), torch.float32)          # no bias
    call(L.kernels(dtype).uclstm_head3x3_fwd, "head3x3_fwd", ad.ptr(), wd.data_ptr(), None, y0.ptr(), N_IMG, H, W, Cp, C, Co)
    ref0, mag0 = RC.head_fwd_ref(a, w, torch.zeros(Co), C)
    assert_within(y0, ref0, (9 * C + 1) * U32 * mag0, "head3x3_fwd no-bias", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("Co", [1, 3])
@pytest.mark.parametrize("C", [16, 10])
@pytest.mark.parametrize("hw", HEAD_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_head3x3_bwd_against_f64(hw, C, Co, dtype):
    H, W, Cp, a, w, b, dy = head_case(hw, C, Co, dtype)
    pixels = N_IMG * H * W
    ad, wd, dyd = put(a), dev32(w), dev32(dy)
    pre_w, pre_b = torch.randn(Co, C, 3, 3) * 0.5, torch.randn(Co) * 0.5          # the kernel adds: attached gradient buffers
    da, dw, db = Guarded((N_IMG, H, W, Cp), dtype), Guarded((Co, C, 3, 3), torch.float32), Guarded((Co,), torch.float32)
    dw.load(pre_w)
    db.load(pre_b)
    geom = (N_IMG, H, W, Cp, C, Co)
    call(L.kernels(dtype).uclstm_head3x3_bwd, "head3x3_bwd", ad.ptr(), wd.data_ptr(), dyd.data_ptr(), da.ptr(), dw.ptr(), db.ptr(), *geom)
    rda, mda, rdw, mdw, rdb, mdb = RC.head_bwd_ref(a, w, dy, C, Cp)
    got_da = assert_within(da, rda, RC.round16_bound(rda, mda, dtype, 9 * Co), "head3x3_bwd da", dtype)
    assert bool((got_da[..., C:] == 0).all())
    assert_within(dw, rdw + pre_w.double(), (pixels + 2) * U32 * (mdw + pre_w.double().abs()), "head3x3_bwd dw", dtype)
    assert_within(db, rdb + pre_b.double(), (pixels + 2) * U32 * (mdb + pre_b.double().abs()), "head3x3_bwd db", dtype)
    # a NULL output is skipped: the others are what they were above, bit for bit where no atomics are involved
    da2 = Guarded((N_IMG, H, W, Cp), dtype)
    call(L.kernels(dtype).uclstm_head3x3_bwd, "head3x3_bwd", ad.ptr(), wd.data_ptr(), dyd.data_ptr(), da2.ptr(), None, None, *geom)
    assert torch.equal(da2.read()[0], got_da)
    dw2 = Guarded((Co, C, 3, 3), torch.float32)
    dw2.load(torch.zeros(Co, C, 3, 3))
    call(L.kernels(dtype).uclstm_head3x3_bwd, "head3x3_bwd", ad.ptr(), wd.data_ptr(), dyd.data_ptr(), None, dw2.ptr(), None, *geom)
    assert_within(dw2, rdw, (pixels + 2) * U32 * mdw, "head3x3_bwd dw-only", dtype)
    db2 = Guarded((Co,), torch.float32)
    db2.load(torch.zeros(Co))
    call(L.kernels(dtype).uclstm_head3x3_bwd, "head3x3_bwd", ad.ptr(), wd.data_ptr(), dyd.data_ptr(), None, None, db2.ptr(), *geom)
    assert_within(db2, rdb, (pixels + 2) * U32 * mdb, "head3x3_bwd db-only", dtype)


def ordered_host_sum(partials, rows, cols, preload):
    """out = (preload) + p[0] + p[1] + ... in f32, left to right (the contract of uclstm_ordered_sum_f32)."""
    acc = np.zeros(cols, dtype=np.float32) if preload is None else preload.numpy().astype(np.float32).reshape(cols).copy()
    p = partials.numpy().astype(np.float32).reshape(rows, cols)
    for r in range(rows):
        acc = (acc + p[r]).astype(np.float32)
    return torch.from_numpy(acc).double()


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("Co", [1, 3])
@pytest.mark.parametrize("C", [16, 10])
@pytest.mark.parametrize("hw", HEAD_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_head3x3_bwd_ordered_is_reproducible_and_in_the_documented_order(hw, C, Co, dtype):
    H, W, Cp, a, w, b, dy = head_case(hw, C, Co, dtype)
    pixels = N_IMG * H * W
    rows = int(L.lib.uclstm_head3x3_bwd_ordered_rows(N_IMG, H, W))
    assert rows == -(-pixels // 2048) and (rows > 1) == (hw == (40, 36))
    ad, wd, dyd = put(a), dev32(w), dev32(dy)
    cols_w, geom = Co * C * 9, (N_IMG, H, W, Cp, C, Co, L.act_type(dtype))
    pre_w, pre_b = torch.randn(Co, C, 3, 3) * 0.5, torch.randn(Co) * 0.5
    rda, mda, rdw, mdw, rdb, mdb = RC.head_bwd_ref(a, w, dy, C, Cp)
    results = []
    for accumulate, rep in itertools.product((0, 1), (0, 1)):
        da, dw, db = Guarded((N_IMG, H, W, Cp), dtype), Guarded((Co, C, 3, 3), torch.float32), Guarded((Co,), torch.float32)
        partials = Guarded((rows * (cols_w + Co),), torch.float32)
        if accumulate:
            dw.load(pre_w)
            db.load(pre_b)
        call(L.lib.uclstm_head3x3_bwd_ordered, "head3x3_bwd_ordered", ad.ptr(), wd.data_ptr(), dyd.data_ptr(), da.ptr(), partials.ptr(), dw.ptr(),
             db.ptr(), accumulate, *geom)
        pw, pb = (pre_w.double(), pre_b.double()) if accumulate else (torch.zeros_like(rdw), torch.zeros_like(rdb))
        assert_within(da, rda, RC.round16_bound(rda, mda, dtype, 9 * Co), "head3x3_bwd_ordered da", dtype)
        gw = assert_within(dw, rdw + pw, (pixels + 2) * U32 * (mdw + pw.abs()), "head3x3_bwd_ordered dw", dtype)
        gb = assert_within(db, rdb + pb, (pixels + 2) * U32 * (mdb + pb.abs()), "head3x3_bwd_ordered db", dtype)
        part, untouched = partials.read()
        assert not bool(untouched.any()), "every element of the partial rows is written"
        assert torch.equal(gw.flatten(), ordered_host_sum(part[:rows * cols_w], rows, cols_w, pre_w if accumulate else None))
        assert torch.equal(gb.flatten(), ordered_host_sum(part[rows * cols_w:], rows, Co, pre_b if accumulate else None))
        results.append((accumulate, da.read()[0], gw, gb, part))
    for (acc0, *r0), (acc1, *r1) in zip(results[0::2], results[1::2]):
        assert acc0 == acc1 and all(torch.equal(x, y) for x, y in zip(r0, r1)), "two calls on the same input differ"
    # NULL outputs: no parameter-gradient launch without dw and db (partials may then be NULL)
    da = Guarded((N_IMG, H, W, Cp), dtype)
    call(L.lib.uclstm_head3x3_bwd_ordered, "head3x3_bwd_ordered", ad.ptr(), wd.data_ptr(), dyd.data_ptr(), da.ptr(), None, None, None, 0, *geom)
    assert torch.equal(da.read()[0], results[0][1])


# ---------------------------------------------------------------------------------------------
# stride-2 descriptors of the implicit-GEMM forward family
# ---------------------------------------------------------------------------------------------
def strided_cases():
    H, W = 5, 6
    for (ktap, pad), N, Cs, odd, stats in itertools.product(((3, 1), (1, 0)), (64, 128), (24, 72), (False, True), (False, True)):
        Hs, Ws = (2 * H - 1, 2 * W - 1) if odd else (2 * H, 2 * W)
        yield IC.Case(f"k{ktap}-N{N}-C{Cs}-{'odd' if odd else 'even'}{'-stats' if stats else ''}", 1 if N <= 64 else 0, N_IMG, H, W,
                      [(Cs, Hs, Ws, 0, 0)], N, ktap=ktap, scale=2, pad=pad, stats=stats, bias=not stats)


STRIDED = list(strided_cases())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", [c.name for c in STRIDED])
def test_stride2_descriptors_against_f64(name, dtype):
    """ktap 3 / scale 2 / pad 1 and ktap 1 / scale 2 / pad 0, N 64 (the 64x256 shape) and 128 (128x128), one and two channel chunks,
    source sizes 2H and 2H - 1, with and without BatchNorm partial sums; bounds and checks of test_store_epilogue_against_f64."""
    c = next(x for x in STRIDED if x.name == name)
    torch.manual_seed(1000 + sum(map(ord, name)))
    Cs, Hs, Ws, _, _ = c.srcs[0]
    assert (Hs - 1) // 2 + 1 == c.H and (Ws - 1) // 2 + 1 == c.W and c.Ktot // (c.ktap ** 2 * 64) == (1 if Cs == 24 else 2)
    x = (torch.randn(c.n_img, Hs, Ws, Cs) * 0.8).to(dtype)
    xd = put(x)
    w = (torch.randn(IC.weight_shape(c)) * (1.6 / (c.ktap * c.ktap * Cs) ** 0.5)).to(DEV)
    wp = ops.pack_weights(IC.pack_desc(c), w, dtype=dtype)
    A = IC.gather_a(c.n_img, c.H, c.W, c.ktap, c.scale, c.pad, [(x, 0, 0)])
    ref, mag = IC.gemm_ref(A, wp.cpu())
    bias = None
    if c.bias:
        bias = torch.randn(c.N) * 0.5
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    bd = None if bias is None else dev32(bias)
    out = Guarded((c.n_img, c.H, c.W, c.N), dtype)
    tiles = IC.stats_tiles(c) if c.stats else None
    stats = Guarded((len(tiles), c.N, 2), torch.float32) if c.stats else None
    d = IC.build_desc(c, [xd.ptr()], wp.data_ptr(), [out.ptr()], None if bd is None else bd.data_ptr(), None, None, stats.ptr() if stats else None)
    shp = int(L.lib.uclstm_igemm_fwd_shape(C.byref(d)))
    assert shp in (0, 1) and shp == c.shape
    T.launch(d, dtype, name)
    got, untouched = out.read()
    check_16bit(got, untouched, ref.view(c.n_img, c.H, c.W, c.N), mag.view(c.n_img, c.H, c.W, c.N), dtype, f"stride-2 {name}",
                f"stride-2 STORE kernel {c.shape}")
    if c.stats:
        assert len(tiles) == int(L.lib.uclstm_igemm_tiles_per_group(c.n_img, c.H, c.W, 1, c.N))
        stored = got.view(c.M, c.N)
        sgot, suntouched = stats.read()
        assert not bool(suntouched.any()), f"{name}: statistics slots not written"
        sref = torch.stack([torch.stack((stored[p].sum(0), (stored[p] ** 2).sum(0)), -1) for p in tiles])
        sabs = torch.stack([torch.stack((stored[p].abs().sum(0), (stored[p] ** 2).sum(0)), -1) for p in tiles])
        e = float(((sgot - sref).abs() / (sabs + 1e-30)).max())
        print(f"[parity] stride-2 {name} stats {tag(dtype)}: max |err| / sum|terms| {e:.2e} (<= 2e-6) over {sref.numel()} sums")
        assert e <= 2e-6, f"{name}: statistics slot off by {e:.3e} of sum|terms|"
