"""The backward kernels of the trainable encoder at the C ABI, in bf16 and fp16, against f64 computed from the device's own stored
inputs (tests/resnet_bwd_cases.py, pinned to autograd by tests/test_resnet_bwd_host.py), and the strided descriptors of the GEMM
families that the encoder's backward pass uses.

Bounds (those of tests/test_gpu_pointwise_abi.py, tests/test_gpu_igemm_abi.py and tests/test_gpu_wgrad_abi.py, none fitted):
  * maxpool3s2_bwd, bn_add_relu_bwd_apply   |err| <= u16*1.01*|ref| + 2^-21*mag + 1e-30    (16-bit element-wise outputs)
  * bn_add_relu_bwd_reduce                  max |err| / sum|terms| <= 2e-6                 (reductions)
  * strided input gradient                  check_16bit of the STORE epilogue              (max(u16*1.01*|ref|, floor) + 2^-21*mag)
  * strided / stem weight gradients         coeff(M, slabs) * mag                          (one f32 rounding per 32 pixels and per slab)
Every 16-bit output sits between guard zones of a NaN pattern and starts out filled with it.  fp16 runs the point-wise backward
kernels on gradients x 1024, as fp16 training does."""

import pytest
import torch

import igemm_cases as IC
import resnet_bwd_cases as BC
import test_gpu_igemm_abi as TI
import test_gpu_pointwise_abi as PW
import test_gpu_wgrad_abi as TW
import wgrad_cases as WC
from test_gpu_igemm_abi import Guarded, tag

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_convlstm_amd import ops
    from unet_convlstm_amd import resnet as R

L = IC.L
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


def put(x, dtype):
    b = Guarded(x.shape, dtype)
    b.load(x)
    return b


def dev32(x):
    return x.float().to(DEV).contiguous()


def call(fn, what, *args):
    L.check(fn(*args, ops._stream()), what)
    torch.cuda.synchronize()


def read_all(buf, what):
    got, untouched = buf.read()                                     # asserts the guard zones
    assert not bool(untouched.any()), f"{what}: {int(untouched.sum())} elements not written"
    return got


# ---------------------------------------------------------------------------------------------
# MaxPool2d(3, 2, 1) backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("use_skip", [True, False], ids=["dskip", "noskip"])
@pytest.mark.parametrize("shape", [(3, 5, 6, 8), (2, 8, 8, 16), (2, 2, 2, 8)], ids=str)
def test_maxpool3s2_bwd_against_f64(shape, use_skip, dtype):
    """da = act16(dskip + the dp of every window whose FIRST maximum sits here): post-ReLU inputs, ties in most windows."""
    n, H, W, Cp = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    a = BC.relu_with_ties(shape, dtype, 31 + H * W)
    assert 0.4 < float((a == 0).float().mean()) < 0.9
    g = torch.Generator().manual_seed(H + W + Cp)
    S = PW.loss_scale(dtype)
    dp = (S * (torch.randn(n, Ho, Wo, Cp, generator=g) + 1.0)).to(dtype)
    dskip = (S * (torch.randn(shape, generator=g) + 1.0)).to(dtype) if use_skip else None
    ad, dpd = put(a, dtype), put(dp, dtype)
    dsd = put(dskip, dtype) if use_skip else None
    K = L.kernels(dtype)
    what = f"maxpool3s2_bwd {shape} {'dskip' if use_skip else 'noskip'} {tag(dtype)}"
    outs = []
    for _ in range(2):
        da = Guarded(shape, dtype)
        call(K.uclstm_maxpool3s2_bwd, "maxpool3s2_bwd", ad.ptr(), dpd.ptr(), dsd.ptr() if use_skip else None, da.ptr(), n, H, W, Cp)
        outs.append(read_all(da, what))
    ref, mag = BC.maxpool3s2_bwd_ref(a, dp, dskip)
    PW.check_elementwise(outs[0], ref, mag, dtype, what)
    assert torch.equal(outs[0], outs[1]), "two launches differ"
    # the pooled gradient is conserved: every window gives its dp to exactly one pixel
    assert torch.allclose(ref.sum((1, 2)) - (dskip.double().sum((1, 2)) if use_skip else 0), dp.double().sum((1, 2)), atol=1e-6 * S)
    # the inputs are untouched (and nothing was written next to them: read() checks the guards)
    assert torch.equal(ad.read()[0], a.double()) and torch.equal(dpd.read()[0], dp.double())


# ---------------------------------------------------------------------------------------------
# relu(bn(z) + bn_r(r)) backward
# ---------------------------------------------------------------------------------------------
TAIL_SHAPES = [(90, 8), (2100, 24), (300, 72)]          # 3, 66 and 10 partial rows; 1, 3 and 9 lanes per pixel
TAIL_CASES = ["both", "identity", "eval_z", "eval_r", "no_dz", "no_dr", "identity_no_dr"]


def tail_inputs(shape, raff, dtype):
    pixels, Cp = shape
    torch.manual_seed(900 + pixels + Cp + int(raff))
    C_ = Cp - 3
    sc, sh, mu, rs = (t[0] for t in PW.bn_params(1, Cp, C_))
    rsc, rsh, rmu, rrs = (t[0] for t in PW.bn_params(1, Cp, C_)) if raff else (None, None, None, None)
    z, r = PW.r16(torch.randn(pixels, Cp), dtype), PW.r16(torch.randn(pixels, Cp), dtype)
    for _ in range(50):                                      # no pre-activation within 1e-4 of the ReLU kink
        u = BC.tail_preactivation(z, sc, sh, r, rsc, rsh)
        near = u.abs() < 1e-4
        near[:, C_:] = False                                 # scale = shift = 0 there: u is 0 or r in any precision
        if not bool(near.any()):
            break
        z[near] = PW.r16(torch.randn(int(near.sum())), dtype)
        r[near] = PW.r16(torch.randn(int(near.sum())) + 0.5, dtype)
    assert not bool(near.any())
    da = PW.r16(PW.loss_scale(dtype) * (torch.randn(pixels, Cp) + 1.0), dtype)
    return dict(sc=sc, sh=sh, mu=mu, rs=rs, rsc=rsc, rsh=rsh, rmu=rmu, rrs=rrs, z=z, r=r, da=da, u=u)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", TAIL_CASES)
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=str)
def test_bn_add_relu_bwd_reduce_and_apply_against_f64(shape, case, dtype):
    pixels, Cp = shape
    raff = not case.startswith("identity")
    c = tail_inputs(shape, raff, dtype)
    K = L.kernels(dtype)
    rows = int(L.lib.uclstm_bn_add_relu_bwd_rows(pixels))
    assert rows == min(1024, -(-pixels // 32)) and rows >= 3
    zd, rd, dad = put(c["z"], dtype), put(c["r"], dtype), put(c["da"], dtype)
    zpar = [dev32(c[k]) for k in ("sc", "sh", "mu", "rs")]
    rpar = [dev32(c[k]) for k in ("rsc", "rsh", "rmu", "rrs")] if raff else [None] * 4
    pz, pr = [t.data_ptr() for t in zpar], [None if t is None else t.data_ptr() for t in rpar]
    what = f"{shape} {case} {tag(dtype)} ({rows} rows)"

    g, xhat, s_ref, s_abs = BC.tail_sums_ref(c["u"], c["z"], c["mu"], c["rs"], c["da"])
    results = []
    for _ in range(2):
        partials, sums = Guarded((rows, Cp, 3), torch.float32), Guarded((Cp, 2), torch.float32)
        rsums = Guarded((Cp, 2), torch.float32) if raff else None
        call(K.uclstm_bn_add_relu_bwd_reduce, "bn_add_relu_bwd_reduce", zd.ptr(), *pz, rd.ptr(), *pr, dad.ptr(), partials.ptr(), sums.ptr(),
             rsums.ptr() if raff else None, pixels, Cp)
        read_all(partials, what + " partials")
        results.append((read_all(sums, what + " sums"), read_all(rsums, what + " rsums") if raff else None))
    sums_got, rsums_got = results[0]
    PW.check_sums(sums_got, s_ref, s_abs, f"bn_add_relu_bwd_reduce sums {what}")
    if raff:
        _, rxhat, rs_ref, rs_abs = BC.tail_sums_ref(c["u"], c["r"], c["rmu"], c["rrs"], c["da"])
        PW.check_sums(rsums_got, rs_ref, rs_abs, f"bn_add_relu_bwd_reduce rsums {what}")
        assert torch.equal(rsums_got[:, 0], sums_got[:, 0])                     # one sum of g for both tables
    assert torch.equal(results[0][0], results[1][0]) and (not raff or torch.equal(results[0][1], results[1][1])), "two launches differ"

    # pass 2 with the sums pass 1 produced (the evaluation-statistics form: zeros for that branch)
    s_z = torch.zeros_like(sums_got) if case == "eval_z" else sums_got
    s_r = None if not raff else (torch.zeros_like(rsums_got) if case == "eval_r" else rsums_got)
    szd, srd = dev32(s_z), None if s_r is None else dev32(s_r)
    want_dz, want_dr = case != "no_dz", case not in ("no_dr", "identity_no_dr")
    outs = []
    for _ in range(2):
        dz = Guarded(shape, dtype) if want_dz else None
        dr = Guarded(shape, dtype) if want_dr else None
        call(K.uclstm_bn_add_relu_bwd_apply, "bn_add_relu_bwd_apply", zd.ptr(), *pz, szd.data_ptr(), rd.ptr(), *pr,
             None if srd is None else srd.data_ptr(), dad.ptr(), dz.ptr() if want_dz else None, dr.ptr() if want_dr else None, pixels, Cp)
        outs.append((read_all(dz, what + " dz") if want_dz else None, read_all(dr, what + " dr") if want_dr else None))
    if want_dz:
        ref, mag = BC.tail_dx_ref(g, xhat, c["z"], c["sc"], c["mu"], c["rs"], s_z.double())
        PW.check_elementwise(outs[0][0], ref, mag, dtype, f"bn_add_relu_bwd_apply dz {what}")
        if case == "eval_z":
            assert torch.equal(ref, c["sc"].double() * g)
    if want_dr and raff:
        ref, mag = BC.tail_dx_ref(g, rxhat, c["r"], c["rsc"], c["rmu"], c["rrs"], s_r.double())
        PW.check_elementwise(outs[0][1], ref, mag, dtype, f"bn_add_relu_bwd_apply dr {what}")
    if want_dr and not raff:
        assert torch.equal(outs[0][1], g), "the identity branch is dr = g, exactly"
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(outs[0], outs[1])), "two launches differ"
    assert torch.equal(zd.read()[0], c["z"].double()) and torch.equal(rd.read()[0], c["r"].double())


# ---------------------------------------------------------------------------------------------
# strided input gradient through the host path
# ---------------------------------------------------------------------------------------------
N_IMG = 3


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("with_ds", [True, False], ids=["ds", "nods"])
@pytest.mark.parametrize("chan", [(64, 128), (128, 256)], ids=lambda v: f"{v[0]}to{v[1]}")
@pytest.mark.parametrize("hw", [(2, 2), (4, 6), (8, 8)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_strided_input_gradient_through_the_host_path(hw, chan, with_ds, dtype):
    """resnet.conv_s2_dgrad: the input gradient of conv3x3 / stride 2 / pad 1 (+ conv1x1 / stride 2 as a second source) as ONE
    forward-family launch, against the GEMM reference on the panel the host packs, which itself is checked against the
    input-gradient identity in f64 (the 16-bit-rounded weights through resnet_bwd_cases.s2_dgrad_ref)."""
    (Hin, Win), (Ci, Co) = hw, chan
    Ho, Wo = Hin // 2, Win // 2
    torch.manual_seed(Hin * Win + Ci + int(with_ds))
    dz = (torch.randn(N_IMG, Ho, Wo, Co) * 0.8).to(dtype)
    dzr = (torch.randn(N_IMG, Ho, Wo, Co) * 0.8).to(dtype) if with_ds else None
    w = torch.randn(Co, Ci, 3, 3) * (1.6 / (9 * Co) ** 0.5)
    wds = torch.randn(Co, Ci, 1, 1) * (1.6 / Co ** 0.5) if with_ds else None
    dzd, dzrd = put(dz, dtype), put(dzr, dtype) if with_ds else None
    wdev, wdsdev = w.to(DEV), wds.to(DEV) if with_ds else None
    ops.LAUNCH_LOG = log = []
    try:
        dx = R.conv_s2_dgrad(dzd.t, wdev, dzrd.t if with_ds else None, wdsdev)
    finally:
        ops.LAUNCH_LOG = None
    torch.cuda.synchronize()
    assert len([e for e in log if e[0] == "fwd"]) == 1, "one launch, no add afterwards"
    assert tuple(dx.shape) == (N_IMG, Hin, Win, Ci) and dx.dtype == dtype
    # the panel the host path packs, and the GEMM reference on it
    pd = R.s2_dgrad_pack_desc(Ci, Co, 2 if with_ds else 1)
    assert pd.Ktot == 4 * Co * (2 if with_ds else 1) and pd.Ktot // 256 == (Co // 64) * (2 if with_ds else 1)
    wp = ops.pack_weights(pd, R.s2_dgrad_weight(wdev, wdsdev), dtype=dtype).cpu()
    A = IC.gather_a(N_IMG, Ho, Wo, 2, 1, 0, [(dz, 0, 0)] + ([(dzr, 0, 0)] if with_ds else []))
    val, mag = IC.gemm_ref(A, wp)
    to_dx = lambda t: t.view(N_IMG, Ho, Wo, 2, 2, Ci).permute(0, 1, 3, 2, 4, 5).reshape(N_IMG, Hin, Win, Ci)
    ref, mag = to_dx(val), to_dx(mag)
    ident = BC.s2_dgrad_ref(dz, w.to(dtype).double(), dzr, None if wds is None else wds.to(dtype).double())
    assert float((ref - ident).abs().max()) <= 1e-9 * float(mag.max()), "the packed panel is not the rearranged weight"
    got = dx.double().cpu()
    TI.check_16bit(got, torch.zeros_like(got, dtype=torch.bool), ref, mag, dtype, f"strided dgrad {hw} {chan} {'ds' if with_ds else 'nods'}",
                   "strided input gradient")


# ---------------------------------------------------------------------------------------------
# strided weight gradients and the stem GEMM
# ---------------------------------------------------------------------------------------------
def wgrad_cases():
    for (Hin, Win) in [(2, 2), (4, 6), (8, 8)]:
        for Ci, Co in [(64, 128), (128, 256)]:
            yield WC.WCase(f"S2-k3-{Hin}x{Win}-{Ci}to{Co}", 0, N_IMG, Hin // 2, Win // 2, [(Ci, Hin, Win, 0, 0)], Co, ktap=3, scale=2, pad=1)
            yield WC.WCase(f"S2-k1-{Hin}x{Win}-{Ci}to{Co}", 0, N_IMG, Hin // 2, Win // 2, [(Ci, Hin, Win, 0, 0)], Co, ktap=1, scale=2, pad=0)
    # the 7x7 stem: a plain GEMM over the saved im2col matrix, K = cpad(49 * 2) = 104 on an 8 x 8 output
    yield WC.WCase("stem-K104-N64", 1, N_IMG, 8, 8, [(104, 8, 8, 0, 0)], 64, ktap=1, scale=1, pad=0)


WGRAD = list(wgrad_cases())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", [c.name for c in WGRAD])
def test_strided_and_stem_weight_gradients_against_f64(name, dtype):
    """ktap 3 / scale 2 / pad 1 and ktap 1 / scale 2 / pad 0 over the OUTPUT grid (the generic kernel) and the stem GEMM (the
    64 x 256 power-of-two kernel), slab mode with the library's own split plan: the f64 sum of the slabs against wgrad_ref."""
    c = next(x for x in WGRAD if x.name == name)
    xs, dys = WC.make_operands(c, dtype)
    ref, mag = WC.case_ref(c, xs, dys)
    xd, dyd = [x.to(DEV).contiguous() for x in xs], [t.to(DEV).contiguous() for t in dys]
    panel = c.N * c.Ktot
    d = WC.build_wgrad_desc(c, [x.data_ptr() for x in xd], [t.data_ptr() for t in dyd], slab=panel)
    assert WC.wgrad_shape(d) == c.shape, f"{name}: kernel {WC.wgrad_shape(d)}, meant for {c.shape}"
    used = WC.wgrad_splits(d)
    assert used >= 1
    d.splits = used
    buf = TW.Guarded(used + 1, panel)
    d.dwp = buf.ptr()
    assert TW.launch(d, dtype) == 0
    got, untouched = buf.read()
    expect = torch.ones_like(untouched)
    expect[:used] = False
    assert torch.equal(untouched, expect), f"{name}: slab elements not written, or written beyond the {used} slabs"
    slabs = got[:used].reshape(used, c.N, c.Ktot)
    assert bool((slabs[:, mag == 0] == 0).all())
    TW.check_panel(slabs.sum(0), ref, mag, None, TW.coeff(c, used), dtype, f"{name} ({used} slabs)", c.shape)
    # through the host wrapper with the model's own descriptor: the same panel gradient
    dwp = ops.igemm_wgrad([ops.SrcView(xd[0])], [(dyd[0], 0, c.N, 0, 1, 0, 0)], c.N, c.Ktot, (c.H, c.W), c.n_img, ktap=c.ktap, scale=c.scale,
                          pad=c.pad)
    torch.cuda.synchronize()
    TW.check_panel(dwp.double().cpu().sum(0), ref, mag, None, TW.coeff(c, dwp.shape[0]), dtype, f"{name} ops.igemm_wgrad", c.shape)
