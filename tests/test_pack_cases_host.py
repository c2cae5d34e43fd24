"""CPU side of tests/test_gpu_pack_abi.py (no GPU, nothing launches).

1. The descriptor builders of ops.py pinned to PyTorch in f64: the panel built from f64 weights through pack_cases.index_map (the
   header's index map, which the GPU tests prove the kernels implement bit for bit), multiplied with the GEMM's A operand as the
   header defines it (igemm_cases.gather_a / scatter_segments / lstm_rows_to_gates), equals F.conv2d / F.conv_transpose2d and
   their autograd gradients at rtol 1e-12.  A flipped tap, a swapped gate or a wrong channel offset in a builder is an O(1) error
   here; through a whole model it moves a rel-L2 by per cent.
2. index_map against igemm_cases.host_panel, two independent restatements of the same header text.
3. The host-side entry points on every case of the table: kernel family and block count of uclstm_pack_job_init, slab groups of
   uclstm_unpack_wgrad_ordered_groups.
4. UCLSTM_E_BADARG for every argument check of the pack / unpack / bias entry points and of uclstm_splitk_finish, with dummy
   pointers.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boundary_cases as BC
import igemm_cases as IC
import pack_cases as PC
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops

F64 = torch.float64
N_IMG, H, W = 2, 3, 4
M = N_IMG * H * W
E_BADARG = -1


def close(got, want, what):
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12, msg=lambda m: f"{what}: {m}")


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def rows(x):
    """[n][C][H][W] -> [pixels][C]"""
    return nhwc(x).reshape(-1, x.shape[1])


def padded(a, n):
    """[M][c] -> [M][n]: random values in the pad columns (the panel or the map must ignore them)."""
    out = torch.randn(a.shape[0], n, dtype=F64)
    out[:, :a.shape[1]] = a
    return out


def zero_padded(a, n):
    out = torch.zeros(a.shape[0], n, dtype=F64)
    out[:, :a.shape[1]] = a
    return out


def gemm(A, d, w, elem_off=0):
    """[M][N]: A times the f64 panel of descriptor d."""
    wp = PC.panel_of(d, w, elem_off)
    assert wp.shape == (d.N, d.Ktot) and A.shape[1] == d.Ktot
    return A @ wp.t()


def unpack64(d, dwp, wshape):
    ref, _, mapped = PC.unpack_ref(d, dwp[None], torch.zeros(wshape, dtype=F64), 0)
    assert bool(mapped.all()), "the unpack descriptor of a whole weight must reach every element"
    return torch.from_numpy(ref).view(wshape)


# ---------------------------------------------------------------------------------------------
# 1. builders pinned to PyTorch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [[5], [5, 3]], ids=str)
def test_conv_panels_equal_conv2d_and_its_gradients(cs):
    torch.manual_seed(11 + len(cs))
    Co, Ci = 6, sum(cs)
    x = torch.randn(N_IMG, Ci, H, W, dtype=F64, requires_grad=True)
    w = torch.randn(Co, Ci, 3, 3, dtype=F64, requires_grad=True)
    y = F.conv2d(x, w, padding=1)
    dy = torch.randn_like(y)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    xs = list(nhwc(x.detach()).split(cs, dim=3))
    # forward
    d = PC.conv_fwd(Co, cs)
    A = IC.gather_a(N_IMG, H, W, 3, 1, 1, [(s, 0, 0) for s in xs])
    out = gemm(A, d, w.detach())
    close(out[:, :Co], rows(y.detach()), "conv forward")
    assert bool((out[:, Co:] == 0).all())
    assert torch.equal(PC.panel_of(d, w.detach()), IC.host_panel(w.detach(), cs, 3, d.N))
    # weight gradient through the same descriptor
    dwp = padded(rows(dy), d.N).t() @ A
    close(unpack64(d, dwp, w.shape), dw, "conv weight gradient")
    # input gradient, per source
    Ady = IC.gather_a(N_IMG, H, W, 3, 1, 1, [(nhwc(dy), 0, 0)])
    ch = 0
    for c in cs:
        dd = ops.conv_dgrad_pack_desc(Co, Ci, c)
        got = gemm(Ady, dd, w.detach(), ch * 9)
        close(got[:, :c], rows(dx[:, ch:ch + c]), f"conv input gradient of source at channel {ch}")
        assert bool((got[:, c:] == 0).all())
        ch += c


@pytest.mark.parametrize("ksize", [1, 3, 5])
def test_lstm_panels_equal_the_gate_convolution_and_its_gradients(ksize):
    torch.manual_seed(20 + ksize)
    Hd, Cx, taps = 5, 3, ksize * ksize
    Hp = ops.cpad(Hd)
    x = torch.randn(N_IMG, Cx, H, W, dtype=F64, requires_grad=True)
    h = torch.randn(N_IMG, Hd, H, W, dtype=F64, requires_grad=True)
    w = torch.randn(4 * Hd, Cx + Hd, ksize, ksize, dtype=F64, requires_grad=True)
    gates = F.conv2d(torch.cat((x, h), 1), w, padding=ksize // 2)                      # [n][4*Hd][H][W], gate-major
    dgp = torch.randn(N_IMG, H, W, 4, Hp, dtype=F64)                                   # dgates [pixels][4][Hd_p], pad columns random
    dg = dgp[..., :Hd].permute(0, 3, 4, 1, 2).reshape(N_IMG, 4 * Hd, H, W)
    dx, dh, dw = torch.autograd.grad(gates, (x, h, w), dg)
    want = gates.detach().view(N_IMG, 4, Hd, H, W).permute(0, 3, 4, 1, 2).reshape(M, 4, Hd)
    wd = w.detach()
    srcs = [(nhwc(x.detach()), 0, 0), (nhwc(h.detach()), 0, 0)]
    # full panel
    d = ops.lstm_pack_desc(Hd, Cx, ksize)
    A = IC.gather_a(N_IMG, H, W, ksize, 1, ksize // 2, srcs)
    pre = gemm(A, d, wd)
    full = IC.lstm_rows_to_gates(pre.contiguous(), Hp)
    close(full[:, :, :Hd], want, "lstm full panel")
    assert bool((full[:, :, Hd:] == 0).all())
    # x half + h half
    halves = sum(gemm(IC.gather_a(N_IMG, H, W, ksize, 1, ksize // 2, [srcs[i]]), ops.lstm_half_pack_desc(Hd, Cx, half, ksize), wd)
                 for i, half in enumerate("xh"))
    close(halves, pre, "lstm x half + h half")
    # input gradients from dgates [pixels][4][Hd_p]
    Adg = IC.gather_a(N_IMG, H, W, ksize, 1, ksize // 2, [(dgp.reshape(N_IMG, H, W, 4 * Hp), 0, 0)])
    for name, cvs, off, ref in (("x", Cx, 0, dx), ("h", Hd, Cx * taps, dh)):
        got = gemm(Adg, ops.lstm_dgrad_pack_desc(Hd, Cx, cvs, ksize), wd, off)
        close(got[:, :cvs], rows(ref), f"lstm input gradient of {name}")
        assert bool((got[:, cvs:] == 0).all())
    # weight gradient: rows = gate*Hd_p + hc, the dgates channel order
    ud = ops.lstm_wgrad_unpack_desc(Hd, Cx, ksize)
    dwp = dgp.reshape(M, 4 * Hp).t() @ A
    close(unpack64(ud, dwp, w.shape), dw, "lstm weight gradient")


@pytest.mark.parametrize("Co", [3, 8])
def test_convt_panels_equal_conv_transpose2d_and_its_gradients(Co):
    torch.manual_seed(30 + Co)
    Ci, Cop = 5, ops.cpad(Co)
    x = torch.randn(N_IMG, Ci, H, W, dtype=F64, requires_grad=True)
    w = torch.randn(Ci, Co, 2, 2, dtype=F64, requires_grad=True)
    u = F.conv_transpose2d(x, w, stride=2)
    du = torch.randn_like(u)
    dx, dw = torch.autograd.grad(u, (x, w), du)
    wd = w.detach()
    # forward: four scale-2 segments, one per tap
    d = ops.convt_pack_desc(Ci, Co)
    A = IC.gather_a(N_IMG, H, W, 1, 1, 0, [(nhwc(x.detach()), 0, 0)])
    out = gemm(A, d, wd)
    dst = torch.stack(IC.scatter_segments(out, N_IMG, H, W, IC._convt_segs(Cop, 2 * H, 2 * W)))
    assert bool(((~dst.isnan()).sum(0) == 1).all()), "every output element is written by exactly one segment"
    dst = dst.nan_to_num(nan=0.0).sum(0)
    close(dst[..., :Co], nhwc(u.detach()), "ConvTranspose forward")
    assert bool((dst[..., Co:] == 0).all())
    # input gradient: 2x2 taps gathered at scale 2
    dd = ops.convt_dgrad_pack_desc(Ci, Co)
    Adu = IC.gather_a(N_IMG, H, W, 2, 2, 0, [(nhwc(du), 0, 0)])
    got = gemm(Adu, dd, wd)
    close(got[:, :Ci], rows(dx), "ConvTranspose input gradient")
    assert bool((got[:, Ci:] == 0).all())
    # weight gradient: dY rows (tap, co)
    dup = torch.randn(N_IMG, 2 * H, 2 * W, Cop, dtype=F64)
    dup[..., :Co] = nhwc(du)
    dyp = torch.cat([dup[:, t // 2::2, t % 2::2, :].reshape(M, Cop) for t in range(4)], 1)
    close(unpack64(d, dyp.t() @ A, w.shape), dw, "ConvTranspose weight gradient")


@pytest.mark.parametrize("Ci", [1, 2, 3])
def test_first_layer_panel_equals_conv2d_on_the_im2col_order(Ci):
    torch.manual_seed(40 + Ci)
    Co, Kp = 6, ops.cpad(9 * Ci)
    x = torch.randn(N_IMG, Ci, H, W, dtype=F64)
    w = torch.randn(Co, Ci, 3, 3, dtype=F64, requires_grad=True)
    y = F.conv2d(x, w, padding=1)
    dy = torch.randn_like(y)
    dw, = torch.autograd.grad(y, w, dy)
    d = ops.im2col_pack_desc(Co, Ci, Kp)
    A = zero_padded(BC.im2col_ref(x, Kp).reshape(M, Kp), d.Ktot)
    out = gemm(A, d, w.detach())
    close(out[:, :Co], rows(y.detach()), "first layer forward")
    assert bool((out[:, Co:] == 0).all())
    A_noisy = padded(BC.im2col_ref(x, Kp).reshape(M, Kp)[:, :9 * Ci], d.Ktot)          # pad taps hold noise: the map must drop them
    close(unpack64(d, padded(rows(dy), d.N).t() @ A_noisy, w.shape), dw, "first layer weight gradient")


def test_conv2x2_dgrad_descriptor_equals_autograd():
    """The hand-filled descriptor of kernel family 4 is what it claims to be: the input-gradient panel of a 2x2 convolution."""
    torch.manual_seed(50)
    Co, Ci = 3, 5
    x = torch.randn(N_IMG, Ci, H, W, dtype=F64, requires_grad=True)
    w = torch.randn(Co, Ci, 2, 2, dtype=F64)
    y = F.conv2d(x, w)                                                                 # [n][Co][H-1][W-1]
    dy = torch.randn_like(y)
    dx, = torch.autograd.grad(y, x, dy)
    d = PC.conv2x2_dgrad_desc(Co, Ci)
    A = IC.gather_a(N_IMG, H, W, 2, 1, 1, [(nhwc(dy), 0, 0)])                          # dy[y + ty - 1][x + tx - 1], zero outside
    got = gemm(A, d, w)
    close(got[:, :Ci], rows(dx), "2x2 conv input gradient")
    assert bool((got[:, Ci:] == 0).all())


# ---------------------------------------------------------------------------------------------
# 2. index_map == host_panel on the table's forward conv cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cs", [("conv fwd c255", [255]), ("conv fwd c256", [256]), ("conv fwd c257", [257]), ("conv fwd 264+24", [264, 24])])
def test_index_map_equals_host_panel(name, cs):
    c = PC.BY_NAME[name]
    torch.manual_seed(60)
    w = torch.randn(c.wshape, dtype=F64)
    d = c.desc
    assert torch.equal(PC.panel_of(d, w), IC.host_panel(w, cs, 3, d.N))


# ---------------------------------------------------------------------------------------------
# 3. host-side entry points on every case
# ---------------------------------------------------------------------------------------------
SLAB_COUNTS = (1, 5, 15, 16, 25, 64, 65, 170, 300)


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
def test_job_init_and_ordered_groups(case):
    d = case.desc
    job = L.PackJob()
    fam = int(L.lib.uclstm_pack_job_init(C.byref(job), C.byref(d), IC.DUMMY, IC.DUMMY, 7))
    assert fam == case.family == job.family, f"{case.name}: kernel family {fam}, the case was written for {case.family}"
    assert job.nblocks == PC.expected_blocks(d, case.family) and job.block0 == 7
    assert bytes(job.d) == bytes(d) and job.w == IC.DUMMY and job.wp == IC.DUMMY
    if case.name == PC.OVER_SWEEP:
        assert d.N * d.Ktot > PC.GENERIC_SWEEP and job.nblocks * 256 == PC.GENERIC_SWEEP
    valid, off = PC.index_map(d)
    assert int((off + case.elem_off)[valid].max()) < int(np.prod(case.wshape)) and int(off[valid].min()) >= 0
    groups = [int(L.lib.uclstm_unpack_wgrad_ordered_groups(C.byref(d), n)) for n in SLAB_COUNTS]
    assert groups == [PC.ordered_groups(d, case.family, n) for n in SLAB_COUNTS], f"{case.name}: {groups}"
    assert all(1 <= g <= 1024 for g in groups)
    if case.family in (PC.FAM_ROWS9, PC.FAM_ROWS4):
        assert groups == [1] * len(SLAB_COUNTS)


def test_the_empty_trailing_group_case_is_what_it_claims():
    d = PC.BY_NAME["first layer ci1"].desc
    g = PC.generic_groups(d, 25)
    per = -(-25 // g)
    assert (g, per) == (6, 5) and (g - 1) * per >= 25                                  # six groups of five: group 5 holds no slab


# ---------------------------------------------------------------------------------------------
# 4. UCLSTM_E_BADARG
# ---------------------------------------------------------------------------------------------
def _bad_descs():
    def mutated(**kw):
        d = PC.conv_fwd(8, [24])
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    good = PC.conv_fwd(8, [24])
    huge = (1 << 31) // good.Ktot + 1
    return {"Ktot != taps * (kseg0 + kseg1)": mutated(Ktot=good.Ktot + 1), "n_mode 3": mutated(n_mode=3), "n_mode -1": mutated(n_mode=-1),
            "k_mode 3": mutated(k_mode=3), "k_mode -1": mutated(k_mode=-1), "nsrc 0": mutated(nsrc=0), "nsrc 3": mutated(nsrc=3),
            "N * Ktot >= 2^31": mutated(N=huge), "N 0": mutated(N=0), "taps 0": mutated(taps=0, Ktot=0),
            "tap-major without n_cp": mutated(n_mode=L.NMODE_TAPMAJOR, n_cp=0), "gates without k_hd": mutated(k_mode=L.KMODE_GATES)}


@pytest.mark.parametrize("what", list(_bad_descs()))
def test_bad_descriptors_are_refused_by_every_entry_point(what):
    d = _bad_descs()[what]
    P, ref = IC.DUMMY, C.byref(d)
    job = L.PackJob()
    for lib in (L.lib, L.lib16):
        assert lib.uclstm_pack_weights(ref, P, P, None) == E_BADARG, what
    assert L.lib.uclstm_pack_job_init(C.byref(job), ref, P, P, 0) == E_BADARG, what
    assert L.lib.uclstm_unpack_wgrad(ref, P, 1, 0, P, 0, None) == E_BADARG, what
    assert L.lib.uclstm_unpack_wgrad_ordered(ref, P, 1, 0, P, P, 0, None) == E_BADARG, what
    assert L.lib.uclstm_unpack_wgrad_ordered_groups(ref, 1) == E_BADARG, what
    assert L.lib.uclstm_pack_bias(ref, P, P, None) == E_BADARG, what


def test_bad_pointers_and_slab_arguments_are_refused():
    d = PC.conv_fwd(8, [24])
    total = d.N * d.Ktot
    P, ref = IC.DUMMY, C.byref(d)
    job = L.PackJob()
    for lib in (L.lib, L.lib16):
        assert lib.uclstm_pack_weights(ref, None, P, None) == E_BADARG
        assert lib.uclstm_pack_weights(ref, P, None, None) == E_BADARG
        assert lib.uclstm_pack_weights(None, P, P, None) == E_BADARG
        assert lib.uclstm_pack_weights_batched(None, 1, 1, 1, None) == E_BADARG
        assert lib.uclstm_pack_weights_batched(P, 0, 1, 1, None) == E_BADARG
        assert lib.uclstm_pack_weights_batched(P, 1, 5, 1, None) == E_BADARG
        assert lib.uclstm_pack_weights_batched(P, 1, -1, 1, None) == E_BADARG
        assert lib.uclstm_pack_weights_batched(P, 1, 1, 0, None) == E_BADARG
    assert L.lib.uclstm_pack_job_init(None, ref, P, P, 0) == E_BADARG
    assert L.lib.uclstm_pack_job_init(C.byref(job), ref, None, P, 0) == E_BADARG
    assert L.lib.uclstm_pack_job_init(C.byref(job), ref, P, None, 0) == E_BADARG
    assert L.lib.uclstm_pack_job_init(C.byref(job), ref, P, P, -1) == E_BADARG
    assert L.lib.uclstm_pack_bias(ref, None, P, None) == E_BADARG
    assert L.lib.uclstm_pack_bias(ref, P, None, None) == E_BADARG
    assert L.lib.uclstm_pack_bias(None, P, P, None) == E_BADARG
    for nslab, slab, dwp, grad in ((0, total, P, P), (-1, total, P, P), (2, total - 1, P, P), (2, 0, P, P), (1, 0, None, P), (1, 0, P, None)):
        assert L.lib.uclstm_unpack_wgrad(ref, dwp, nslab, slab, grad, 0, None) == E_BADARG, (nslab, slab)
        assert L.lib.uclstm_unpack_wgrad_ordered(ref, dwp, nslab, slab, None, grad, 0, None) == E_BADARG, (nslab, slab)
    assert L.lib.uclstm_unpack_wgrad_ordered_groups(ref, 0) == E_BADARG
    # several groups: the scratch is required, and the slab stride is checked even though nslab > 1 is implied
    g = PC.BY_NAME["first layer ci1"].desc
    assert int(L.lib.uclstm_unpack_wgrad_ordered_groups(C.byref(g), 300)) > 1
    assert L.lib.uclstm_unpack_wgrad_ordered(C.byref(g), P, 300, g.N * g.Ktot, None, P, 1, None) == E_BADARG
    assert L.lib.uclstm_unpack_wgrad_ordered(C.byref(g), P, 300, g.N * g.Ktot - 1, P, P, 1, None) == E_BADARG


SPLITK_BAD = {
    # (pre, nslab, slab, ld, out, pixels, C)
    "unaligned pre": (IC.DUMMY + 4, 2, 16 * 24, 24, IC.DUMMY, 16, 24),
    "unaligned out": (IC.DUMMY, 2, 16 * 24, 24, IC.DUMMY + 2, 16, 24),
    "NULL pre": (None, 2, 16 * 24, 24, IC.DUMMY, 16, 24),
    "NULL out": (IC.DUMMY, 2, 16 * 24, 24, None, 16, 24),
    "ld < C": (IC.DUMMY, 2, 16 * 24, 20, IC.DUMMY, 16, 24),
    "ld % 4": (IC.DUMMY, 2, 16 * 26, 26, IC.DUMMY, 16, 24),
    "C % 8": (IC.DUMMY, 2, 16 * 12, 12, IC.DUMMY, 16, 12),
    "slab % 4": (IC.DUMMY, 2, 16 * 24 + 2, 24, IC.DUMMY, 16, 24),
    "slab < pixels * ld": (IC.DUMMY, 2, 16 * 24 - 4, 24, IC.DUMMY, 16, 24),
    "nslab 0": (IC.DUMMY, 0, 16 * 24, 24, IC.DUMMY, 16, 24),
    "pixels 0": (IC.DUMMY, 1, 0, 24, IC.DUMMY, 0, 24),
    "C 0": (IC.DUMMY, 1, 0, 24, IC.DUMMY, 16, 0),
    "2^31 chunks": (IC.DUMMY, 1, 0, 8, IC.DUMMY, 1 << 31, 8),
}


@pytest.mark.parametrize("what", list(SPLITK_BAD))
def test_splitk_finish_refuses_bad_arguments(what):
    pre, nslab, slab, ld, out, pixels, Cc = SPLITK_BAD[what]
    for lib in (L.lib, L.lib16):
        assert lib.uclstm_splitk_finish(pre, nslab, slab, ld, IC.DUMMY, IC.DUMMY, IC.DUMMY, 1, out, pixels, Cc, None) == E_BADARG, what


def test_splitk_cases_are_what_they_claim():
    for case in PC.SPLITK_CASES:
        pixels, Cc, ld, nslab, extra, relu, _ = case
        assert Cc % 8 == 0 and ld >= Cc and ld % 4 == 0 and (pixels * ld + extra) % 4 == 0
    assert {c[3] for c in PC.SPLITK_CASES} == {1, 2, 3, 8} and {c[1] for c in PC.SPLITK_CASES} == {8, 24, 512}
    assert len({c[6] for c in PC.SPLITK_CASES}) == 8
    pre, body, bias, scale, shift = PC.splitk_input(PC.SPLITK_CASES[4], torch.bfloat16)
    assert bool(pre.view(3, 37, 28)[:, :, 24:].isnan().all()) and bool((scale < 0).any())
    ref, mag = PC.splitk_finish_ref(pre.view(3, 37, 28), bias, scale, shift, 1, 24)
    want = torch.relu((body.double().sum(0) + bias.double()) * scale.double() + shift.double())
    close(ref, want, "splitk_finish_ref")
    assert bool((mag >= ref.abs()).all())


# ---------------------------------------------------------------------------------------------
# ops.conv_pack_desc is the one builder of both models' convolutions: its fields against those of the two builders it replaced
# (ops.conv_pack_desc for 9 taps, resnet.conv_desc for one source and any tap count), recorded from them as literals
# ---------------------------------------------------------------------------------------------
def _fields(d):
    out = []
    for name, _ in L.PackDesc._fields_:
        v = getattr(d, name)
        out += list(v) if hasattr(v, "__len__") else [v]
    return tuple(out)


CHOFF1 = 9          # choff[1] in _fields: the old builders disagreed for one source (0 / c_valid[0]); the kernels read it for two only
# (Co, Ci, k) of every convolution of ResNet18 behind the stem, as resnet.conv_desc(Co, Ci, k, cpad(Ci)) built them
RESNET18_DESCS = [
    ((64, 64, 3), (64, 576, 9, 1, 64, 0, 64, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 576, 9, 1, 0)),
    ((128, 64, 3), (128, 576, 9, 1, 64, 0, 64, 0, 0, 0, 0, 128, 0, 0, 0, 0, 0, 576, 9, 1, 0)),
    ((128, 128, 3), (128, 1152, 9, 1, 128, 0, 128, 0, 0, 0, 0, 128, 0, 0, 0, 0, 0, 1152, 9, 1, 0)),
    ((128, 64, 1), (128, 64, 1, 1, 64, 0, 64, 0, 0, 0, 0, 128, 0, 0, 0, 0, 0, 64, 1, 1, 0)),
    ((256, 128, 3), (256, 1152, 9, 1, 128, 0, 128, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 1152, 9, 1, 0)),
    ((256, 256, 3), (256, 2304, 9, 1, 256, 0, 256, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 2304, 9, 1, 0)),
    ((256, 128, 1), (256, 128, 1, 1, 128, 0, 128, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 128, 1, 1, 0)),
    ((512, 256, 3), (512, 2304, 9, 1, 256, 0, 256, 0, 0, 0, 0, 512, 0, 0, 0, 0, 0, 2304, 9, 1, 0)),
    ((512, 512, 3), (512, 4608, 9, 1, 512, 0, 512, 0, 0, 0, 0, 512, 0, 0, 0, 0, 0, 4608, 9, 1, 0)),
    ((512, 256, 1), (512, 256, 1, 1, 256, 0, 256, 0, 0, 0, 0, 512, 0, 0, 0, 0, 0, 256, 1, 1, 0)),
]
# (Co, valid channels per source) of the conv cases of pack_cases.CASES / test_gpu_pack.py, as the 9-tap ops.conv_pack_desc built them
STAGE_DESCS = [
    ((8, (255,)), (8, 2304, 9, 1, 256, 0, 255, 0, 0, 255, 0, 8, 0, 0, 0, 0, 0, 2295, 9, 1, 0)),
    ((8, (256,)), (8, 2304, 9, 1, 256, 0, 256, 0, 0, 256, 0, 8, 0, 0, 0, 0, 0, 2304, 9, 1, 0)),
    ((8, (257,)), (8, 2880, 9, 1, 320, 0, 257, 0, 0, 257, 0, 8, 0, 0, 0, 0, 0, 2313, 9, 1, 0)),
    ((8, (264, 24)), (8, 3456, 9, 2, 320, 64, 264, 24, 0, 264, 0, 8, 0, 0, 0, 0, 0, 2592, 9, 1, 0)),
    ((40, (24,)), (40, 576, 9, 1, 64, 0, 24, 0, 0, 24, 0, 40, 0, 0, 0, 0, 0, 216, 9, 1, 0)),
    ((72, (56, 24)), (72, 1152, 9, 2, 64, 64, 56, 24, 0, 56, 0, 72, 0, 0, 0, 0, 0, 720, 9, 1, 0)),
    ((64, (64,)), (64, 576, 9, 1, 64, 0, 64, 0, 0, 64, 0, 64, 0, 0, 0, 0, 0, 576, 9, 1, 0)),
]


def test_the_one_conv_descriptor_builder_equals_both_builders_it_replaced():
    def same(got, want, what, one_source):
        assert len(got) == len(want) == 21
        for i, (g, w) in enumerate(zip(got, want)):
            if i == CHOFF1 and one_source:
                assert g == 0, f"{what}: choff[1] of a one-source descriptor is 0"
                continue
            assert g == w, f"{what}: field {i} of _fields is {g}, the replaced builder had {w}"

    for (Co, Ci, k), want in RESNET18_DESCS:
        same(_fields(ops.conv_pack_desc(Co, Ci, (Ci,), (ops.cpad(Ci),), k)), want, f"ResNet18 {Co} x {Ci} x {k} x {k}", True)
    for (Co, cs), want in STAGE_DESCS:
        same(_fields(ops.conv_pack_desc(Co, sum(cs), cs, [ops.cpad(c) for c in cs])), want, f"stage {Co} x {cs}", len(cs) == 1)
    assert [(Co, cs) for (Co, cs), _ in STAGE_DESCS[:4]] == [(8, (255,)), (8, (256,)), (8, (257,)), (8, (264, 24))]
    # and the descriptor the models get is this builder's: geometry of a 1x1 / stride 2 downsample convolution
    import types
    x, w = types.SimpleNamespace(shape=(2, 8, 8, 64)), types.SimpleNamespace(shape=(128, 64, 1, 1))
    real, ops.SrcView = ops.SrcView, lambda t, *a: t
    try:
        pd, srcs, ktap, scale, pad, Ho, Wo = ops.conv_geometry(x, None, w, (64,), (0, 0), None, 2)
    finally:
        ops.SrcView = real
    assert _fields(pd)[:CHOFF1] == RESNET18_DESCS[3][1][:CHOFF1] and (ktap, scale, pad, Ho, Wo) == (1, 2, 0, 4, 4) and srcs == [x]
