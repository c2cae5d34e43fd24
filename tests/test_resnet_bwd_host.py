"""CPU-only tests of the trainable encoder (csrc/resnet_bwd.hip, the backward half of unet-convlstm_amd/resnet.py): the f64
references of tests/resnet_bwd_cases.py against torch's own autograd, the rearranged weight of the strided input gradient, the C ABI
of the new entry points (declared, bound, exported, every argument contract a code before any launch) and the opt-in interface.
No kernel is launched here."""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

import resnet_bwd_cases as BC
from resnet_cases import nchw, nhwc

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import build as B
from unet_convlstm_amd import resnet as R

TWINS = ["uclstm_maxpool3s2_bwd", "uclstm_bn_add_relu_bwd_reduce", "uclstm_bn_add_relu_bwd_apply"]
ONCE = ["uclstm_bn_add_relu_bwd_rows"]
P = 1 << 20          # an aligned dummy pointer


# ---------------------------------------------------------------------------------------------
# the references against autograd in f64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 6, 8), (2, 8, 8, 16), (2, 2, 2, 8), (1, 7, 9, 8)], ids=str)
@pytest.mark.parametrize("use_skip", [True, False], ids=["dskip", "noskip"])
def test_maxpool_reference_is_autograd_of_max_pool2d(shape, use_skip):
    n, H, W, Cc = shape
    a = BC.relu_with_ties(shape, torch.float64, 11 + H)
    g = torch.Generator().manual_seed(H * W)
    dp = torch.randn(n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, generator=g, dtype=torch.float64)
    dskip = torch.randn(shape, generator=g, dtype=torch.float64) if use_skip else None
    leaf = nchw(a).clone().requires_grad_(True)
    p = F.max_pool2d(leaf, 3, 2, 1)
    # exact ties in most windows: the reference's first-maximum rule has to be ATen's for this to agree
    cols = F.unfold(F.pad(nchw(a), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(n, Cc, 9, -1)
    assert float(((cols == cols.max(2, keepdim=True).values).sum(2) > 1).double().mean()) > 0.3
    (auto,) = torch.autograd.grad(p, leaf, nchw(dp))
    if use_skip:
        auto = auto + nchw(dskip)
    ref, mag = BC.maxpool3s2_bwd_ref(a, dp, dskip)
    assert torch.equal(ref, nhwc(auto)) or float((ref - nhwc(auto)).abs().max()) < 1e-14
    assert bool((mag >= ref.abs() - 1e-14).all())


@pytest.mark.parametrize("raff", [True, False], ids=["bn_r", "identity"])
def test_tail_reference_is_autograd_of_batch_norm_add_relu(raff):
    torch.manual_seed(5)
    n, Cc = 90, 8
    z, r, da = (torch.randn(n, Cc, dtype=torch.float64) for _ in range(3))
    gam, bet, rgam, rbet = (torch.randn(Cc, dtype=torch.float64) for _ in range(4))
    leaves = [t.clone().requires_grad_(True) for t in (z, r, gam, bet, rgam, rbet)]
    zl, rl, g1, b1, g2, b2 = leaves
    u = F.batch_norm(zl, None, None, g1, b1, True, 0.1, 1e-5) + (F.batch_norm(rl, None, None, g2, b2, True, 0.1, 1e-5) if raff else rl)
    grads = torch.autograd.grad(F.relu(u), leaves[:4] + (leaves[4:] if raff else []), da)

    def consts(x, gamma, beta):
        mean, rstd = x.mean(0), (x.var(0, unbiased=False) + 1e-5).rsqrt()
        return gamma * rstd, beta - mean * gamma * rstd, mean, rstd

    sc, sh, mu, rs = consts(z, gam, bet)
    rsc, rsh, rmu, rrs = consts(r, rgam, rbet) if raff else (None, None, None, None)
    pre = BC.tail_preactivation(z, sc, sh, r, rsc, rsh)
    assert torch.allclose(pre, u.detach(), atol=1e-12)
    g, xhat, sums, mags = BC.tail_sums_ref(pre, z, mu, rs, da)
    dz, _ = BC.tail_dx_ref(g, xhat, z, sc, mu, rs, sums)
    assert torch.allclose(dz, grads[0], atol=1e-12) and bool((mags >= sums.abs() - 1e-12).all())
    assert torch.allclose(sums[:, 1], grads[2], atol=1e-12) and torch.allclose(sums[:, 0], grads[3], atol=1e-12)          # dgamma, dbeta
    if raff:
        _, rxhat, rsums, _ = BC.tail_sums_ref(pre, r, rmu, rrs, da)
        dr, _ = BC.tail_dx_ref(g, rxhat, r, rsc, rmu, rrs, rsums)
        assert torch.allclose(dr, grads[1], atol=1e-12)
        assert torch.allclose(rsums[:, 1], grads[4], atol=1e-12) and torch.allclose(rsums[:, 0], grads[5], atol=1e-12)
        # evaluation statistics (constants): zero sums give scale * g
        ez, _ = BC.tail_dx_ref(g, xhat, z, sc, mu, rs, torch.zeros_like(sums))
        assert torch.equal(ez, sc * g)
    else:
        assert torch.allclose(g, grads[1], atol=1e-12)                                                                    # dr = g


@pytest.mark.parametrize("with_ds", [True, False], ids=["ds", "nods"])
@pytest.mark.parametrize("hw", [(2, 2), (4, 6), (8, 8)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_rearranged_weight_gives_the_input_gradient_of_the_strided_convolutions(hw, with_ds):
    Hin, Win = hw
    torch.manual_seed(Hin * Win)
    n, Ci, Co = 2, 5, 7
    x = torch.randn(n, Ci, Hin, Win, dtype=torch.float64, requires_grad=True)
    w, wds = torch.randn(Co, Ci, 3, 3, dtype=torch.float64), torch.randn(Co, Ci, 1, 1, dtype=torch.float64)
    z = F.conv2d(x, w, None, 2, 1)
    dz = torch.randn_like(z)
    outs, gouts = [z], [dz]
    dzr = None
    if with_ds:
        zr = F.conv2d(x, wds, None, 2, 0)
        dzr = torch.randn_like(zr)
        outs, gouts = outs + [zr], gouts + [dzr]
    (auto,) = torch.autograd.grad(outs, x, gouts)
    wr = R.s2_dgrad_weight(w, wds if with_ds else None)
    assert wr.dtype == w.dtype and tuple(wr.shape) == (Co * (2 if with_ds else 1), Ci, 2, 2, 2, 2) and wr.is_contiguous()
    assert int((wr[:Co] != 0).sum()) == 9 * Co * Ci                                    # 9 of the 16 (parity, tap) slots are used
    got = BC.s2_dgrad_ref(nhwc(dz), w, None if dzr is None else nhwc(dzr), wds if with_ds else None)
    assert float((nchw(got) - auto).abs().max()) < 1e-12
    d = R.s2_dgrad_pack_desc(Ci, Co, 2 if with_ds else 1)
    assert (d.N, d.taps, d.Ktot) == (4 * 8, 4, 4 * 64 * (2 if with_ds else 1)) and d.n_mode == L.NMODE_TAPMAJOR


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_entry_points():
    hdr = open(L.HEADER_PATH).read()
    syms = set(L.header_symbols())
    raw = C.CDLL(L.LIB_PATH)
    listed = re.search(r"#define UCLSTM_RESNET_BWD_F16_TWINS\(TWIN\)(.*?)\nUCLSTM_RESNET_BWD_F16_TWINS\(UCLSTM_F16_TWIN\)", hdr, re.S)
    assert listed, "the twins of csrc/resnet_bwd.hip are declared through UCLSTM_F16_TWIN"
    assert re.findall(r"TWIN\((uclstm_[a-z0-9_]+)\)", listed.group(1)) == TWINS == L.RESNET_BWD_F16_TWINS
    assert hdr.index("UCLSTM_RESNET_F16_TWINS(UCLSTM_F16_TWIN)") < hdr.index("#define UCLSTM_RESNET_BWD_F16_TWINS")
    for name in TWINS + ONCE:
        assert name in syms and name in L._PROTOS and hasattr(raw, name), name
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr).group(1)
        assert len([a for a in params.split(",") if a.strip()]) == len(L._PROTOS[name]), name
    for name in TWINS:
        assert hasattr(raw, name + "_f16"), name
        assert getattr(L.kernels(torch.float16), name) is not getattr(L.lib, name)
    for name in ONCE:
        assert not hasattr(raw, name + "_f16")
    assert L._RESTYPES["uclstm_bn_add_relu_bwd_rows"] is C.c_int64
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16 == int(re.search(r"#define UCLSTM_ABI_VERSION (\d+)", hdr).group(1))
    assert "resnet_bwd.hip" in B.SOURCES and "resnet_bwd.hip" in B.F16_SOURCES


@pytest.mark.parametrize("lib", [L.lib, L.lib16], ids=["bf16", "fp16"])
def test_every_argument_check_is_a_code_before_any_launch(lib):
    E = -1
    # maxpool3s2_bwd(a, dp, dskip, da, n_img, H, W, Cp, stream)
    f = lib.uclstm_maxpool3s2_bwd
    for args in [(None, P, P, P, 3, 5, 6, 8), (P, None, P, P, 3, 5, 6, 8), (P, P, P, None, 3, 5, 6, 8), (P + 2, P, P, P, 3, 5, 6, 8),
                 (P, P + 2, P, P, 3, 5, 6, 8), (P, P, P + 2, P, 3, 5, 6, 8), (P, P, None, P + 2, 3, 5, 6, 8), (P, P, P, P, 0, 5, 6, 8),
                 (P, P, P, P, 3, 0, 6, 8), (P, P, P, P, 3, 5, 0, 8), (P, P, P, P, 3, 5, 6, 0), (P, P, P, P, 3, 5, 6, 12),
                 (P, P, P, P, 1 << 16, 256, 256, 64)]:
        assert f(*args, None) == E, args
    # bn_add_relu_bwd_reduce(z, scale, shift, mean, rstd, r, rscale, rshift, rmean, rrstd, da, partials, sums, rsums, pixels, Cp, stream)
    f = lib.uclstm_bn_add_relu_bwd_reduce
    ok = [P] * 14 + [90, 8]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 5, 10, 11, 12)] + [(i, P + 4) for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)]
    bad += [(i, None) for i in (6, 7, 8, 9, 13)]                       # the BatchNorm of r: all five or none
    bad += [(14, 0), (15, 0), (15, 20), (15, 8 * 257), (14, 1 << 31)]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert f(*args, None) == E, (i, v)
    ident = list(ok)
    for i in (6, 7, 8, 9):
        ident[i] = None
    assert f(*ident, None) == E                                      # rsums without the BatchNorm of r
    # bn_add_relu_bwd_apply(z, scale, shift, mean, rstd, sums, r, rscale, rshift, rmean, rrstd, rsums, da, dz, dr, pixels, Cp, stream)
    f = lib.uclstm_bn_add_relu_bwd_apply
    ok = [P] * 15 + [90, 8]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 5, 6, 12)] + [(i, P + 4) for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14)]
    bad += [(i, None) for i in (7, 8, 9, 10, 11)] + [(15, 0), (16, 0), (16, 20), (16, 8 * 257), (15, 1 << 31)]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert f(*args, None) == E, (i, v)
    none = list(ok)
    none[13] = none[14] = None
    assert f(*none, None) == E                                       # neither dz nor dr
    rows = L.lib.uclstm_bn_add_relu_bwd_rows
    assert rows(0) == E and rows(-5) == E
    sizes = [1, 32, 33, 90, 32 * 1024, 32 * 1024 + 1, 1 << 24]
    assert [int(rows(n)) for n in sizes] == [min(1024, -(-n // 32)) for n in sizes]


# ---------------------------------------------------------------------------------------------
# the opt-in interface
# ---------------------------------------------------------------------------------------------
def enc_names(m, flag=True):
    return {k for k, p in m.encoder.named_parameters() if p.requires_grad == flag}


def test_unfreeze_encoder_sets_requires_grad_by_stage():
    m = U.PretrainedTemporalUNet(lstm_layers=2)
    every = {k for k, _ in m.encoder.named_parameters()}
    assert enc_names(m) == set() and not m._encoder_opt_in
    assert m.unfreeze_encoder("all") is m and enc_names(m) == every and m._encoder_opt_in
    m.unfreeze_encoder(("layer3", "layer4"))
    assert enc_names(m) == {k for k in every if k.startswith(("layer3.", "layer4."))} and len(enc_names(m)) == 30
    m.unfreeze_encoder("stem")
    assert enc_names(m) == {"conv1.weight", "bn1.weight", "bn1.bias"}
    m.unfreeze_encoder(())
    assert enc_names(m) == set() and m._encoder_opt_in and m._first_trainable_stage() is None
    m.unfreeze_encoder()                                               # the default is "all"
    assert enc_names(m) == every and m._first_trainable_stage() == 0
    for bad in ("layer5", ("layer1", "fc"), "encoder"):
        with pytest.raises(U.UclstmError, match="unknown encoder stage"):
            m.unfreeze_encoder(bad)
    assert enc_names(m) == every                                       # a refused call changes nothing
    # nothing outside the encoder is touched; lstm_skips.0 stays out
    outside = {k: p.requires_grad for k, p in m.named_parameters() if ".encoder." not in k and not k.startswith("encoder.")}
    assert all(v == (not k.startswith("lstm_skips.0.")) for k, v in outside.items())
    # single parameters may be toggled afterwards: the lowest trainable stage follows
    m.unfreeze_encoder(("layer4",))
    assert m._first_trainable_stage() == 4
    m.encoder.layer2[1].bn2.bias.requires_grad = True
    assert m._first_trainable_stage() == 2
    # the state_dict does not change
    assert set(m.state_dict()) == set(U.PretrainedTemporalUNet(lstm_layers=2).state_dict())


def test_without_the_opt_in_the_guard_stays():
    class FakeDevice(torch.Tensor):
        is_cuda = True

    x = torch.zeros(1, 2, 2, 64, 64).as_subclass(FakeDevice)
    unfrozen = U.PretrainedTemporalUNet(freeze_encoder=False)
    with pytest.raises(U.UclstmError, match="unfrozen encoder") as e:
        unfrozen(x)
    assert "unfreeze_encoder" in str(e.value)
    m = U.PretrainedTemporalUNet()
    m.encoder.layer4[1].bn2.weight.requires_grad = True                 # by hand, without the method: still refused
    with pytest.raises(U.UclstmError, match="unfrozen encoder"):
        m(x)
