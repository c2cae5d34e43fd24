"""The reference's shipped model, train/resnet18.py: a ResNet18 encoder, five ConvLSTMs and smp's UNet decoder, on libuclstm.so.

``PretrainedTemporalUNet`` keeps the reference's constructor, attribute names and ``state_dict`` keys (those of
``smp.Unet("resnet18", in_channels=2, decoder_channels=(256, 128, 64, 32, 16))`` registered twice, as
``train/resnet18.py:26-38`` does, plus ``lstm`` and ``lstm_skips``), so a ``resnet18_frozen_*`` checkpoint loads with
``strict=True``.  Neither ``segmentation_models_pytorch`` nor ``torchvision`` is imported: the containers are stock
``nn.Conv2d`` / ``nn.BatchNorm2d`` modules that are never called, and every forward goes through HIP kernels -- the
implicit-GEMM family for the convolutions (stride 2 is a descriptor with ``scale = 2``), ``ops.ConvBNReLU`` for the decoder
stages, this package's ``ConvLSTM`` for the recurrences and the kernels of ``csrc/resnet.hip`` around them.

The encoder has ONE route (``_encode`` / ``_block`` / ``_conv_bn``), and every forward body is a plain function without autograd:
those of ops.py that ``ops.ConvBNReLU`` runs on too -- ``ops.conv_bn_stats`` (convolution + BatchNorm constants), ``ops.conv_bn_fold``
(evaluation statistics in the GEMM's epilogue), ``ops.bn_relu``, all on the one ``ops.conv_geometry`` -- and ``bn_add_relu``,
``maxpool3s2`` here.  A frozen stage calls them directly.  After
``model.unfreeze_encoder(stages)`` the stages from the lowest trainable one up call them through the autograd Functions ``EncConv``,
``BnRelu``, ``BnAddRelu``, ``MaxPool3s2``, whose backward is the kernels of ``csrc/resnet_bwd.hip``, the stride-2 weight gradients as
descriptors of the weight-gradient family over the OUTPUT grid, and the stride-2 input gradient as one launch of the forward family
over the four parities of the input pixel (``conv_s2_dgrad``).  Each BatchNorm decides by its own mode; the fold is taken exactly when
it uses its running statistics and its stage is not under autograd (with a backward pass ``z`` is kept and BatchNorm applied after it).

Frame-by-frame inference is ``step_nhwc`` (driven by ``streaming.PretrainedStreamingPredictor``): the five recurrences advance
layer by layer, each layer of all five as one ``ops.convlstm_tick``.

Not part of this module: ``GraphedTrainStep`` and ``sync_batchnorm`` with this model, and a fused upsample.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import modules, ops
from ._lib import UclstmError
from .modules import ConvLSTM, bn_mode
from .ops import F32, SrcView, _p, _stream, cpad, kseg

Tensor = torch.Tensor

ENCODER_CHANNELS = (2, 64, 64, 128, 256, 512)          # smp's resnet18 encoder.out_channels with in_channels = 2
DECODER_CHANNELS = (256, 128, 64, 32, 16)              # train/resnet18.py:32
HEAD_MAX_OUT = 4                                       # uclstm_head3x3_*: output channels are register accumulators
ENCODER_STAGES = ("stem", "layer1", "layer2", "layer3", "layer4")          # what unfreeze_encoder() names

# LAUNCH_LOG kinds of the head's parameter-gradient reduction, next to ops.ATOMIC_KINDS / ops.ORDERED_KINDS
ATOMIC_KINDS = ops.ATOMIC_KINDS + ("head3x3_bwd",)
ORDERED_KINDS = ops.ORDERED_KINDS + ("head3x3_bwd_ordered",)


# ---------------------------------------------------------------------------------------------
# parameter containers (the reference's key layout; never called)
# ---------------------------------------------------------------------------------------------
class BasicBlock(nn.Module):
    """torchvision's BasicBlock: ``relu(bn2(conv2(relu(bn1(conv1(x))))) + identity)``, identity through ``downsample`` if present."""

    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))


class ResNet18Encoder(nn.Module):
    """``resnet18`` without ``fc`` / ``avgpool`` and with a 2-channel ``conv1`` (smp's ResNetEncoder)."""

    def __init__(self, in_channels: int = 2):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        widths = (64, 128, 256, 512)
        cin = 64
        for i, w in enumerate(widths):
            setattr(self, f"layer{i + 1}", nn.Sequential(BasicBlock(cin, w, 1 if i == 0 else 2), BasicBlock(w, w, 1)))
            cin = w
        self.out_channels = ENCODER_CHANNELS


class DecoderBlock(nn.Module):
    """smp's DecoderBlock: nearest x2, cat([x, skip]), (conv3x3 no bias, BatchNorm, ReLU) twice; the attentions are identities."""

    def __init__(self, cin: int, cskip: int, cout: int):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(cin + cskip, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.attention1 = nn.Identity()
        self.conv2 = nn.Sequential(nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.attention2 = nn.Identity()
        self.channels = (cin, cskip, cout)


class UnetDecoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.center = nn.Identity()
        ins = (ENCODER_CHANNELS[-1],) + DECODER_CHANNELS[:-1]
        skips = ENCODER_CHANNELS[1:-1][::-1] + (0,)
        self.blocks = nn.ModuleList(DecoderBlock(i, s, o) for i, s, o in zip(ins, skips, DECODER_CHANNELS))


class _BaseModel(nn.Module):
    """The ``smp.Unet`` the reference keeps as ``base_model``: only a namespace for the three parts."""

    def __init__(self, out_channels: int):
        super().__init__()
        self.encoder = ResNet18Encoder(2)
        self.decoder = UnetDecoder()
        self.segmentation_head = nn.Sequential(nn.Conv2d(DECODER_CHANNELS[-1], out_channels, 3, padding=1), nn.Identity(), nn.Identity())


def adapt_first_conv(w: Tensor) -> Tensor:
    """smp's rule for ``in_channels = 2``: the first two input channels of the 3-channel ImageNet filter, scaled by 3/2."""
    return w if w.shape[1] == 2 else w[:, :2] * 1.5


# ---------------------------------------------------------------------------------------------
# host wiring of csrc/resnet.hip
# ---------------------------------------------------------------------------------------------
def im2col7_pack_desc(Co: int, Ci: int, Kp: int) -> L.PackDesc:
    """Panel of the pre-gathered 7x7 first layer: K = (tap, ci), 49 taps (ops.im2col_pack_desc for the 3x3 one)."""
    d = ops.im2col_pack_desc(Co, Ci, Kp)
    d.cvalid[0] = 49 * Ci
    d.k_hdp = 49
    d.stride_n, d.stride_k = Ci * 49, 49
    return d


def im2col7x7s2_first(x: Tensor) -> Tensor:
    """f32 ``[B,T,C,H,W]`` -> 16-bit ``[T*B, Ho, Wo, Kp]`` (image ``t*B + b``), K = (tap, c) of the 7x7 / stride 2 / pad 3 conv."""
    ops._dev(x, F32, "input")
    B, T, Cc, H, W = x.shape
    Kp = cpad(49 * Cc)
    out = torch.empty((B * T, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Kp), dtype=ops.get_compute_dtype(), device=x.device)
    L.check(ops._k(out).uclstm_im2col7x7s2_first(_p(x), _p(out), B * T, Cc, Kp, H, W, B, Cc * H * W, T * Cc * H * W, _stream()),
            "im2col7x7s2_first")
    return out


def maxpool3s2(a: Tensor) -> Tensor:
    ops._dev(a, ops.ACT, "activation")
    N, H, W, Cp = a.shape
    p = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cp), dtype=a.dtype, device=a.device)
    ops._timed_hbm("maxpool3s2_fwd", 2.0 * (a.numel() + p.numel()),
                   lambda: L.check(ops._k(a).uclstm_maxpool3s2_fwd(_p(a), _p(p), N, H, W, Cp, _stream()), "maxpool3s2_fwd"))
    return p


def bn_add_relu(z: Tensor, par: Optional[Tensor], r: Tensor, rpar: Optional[Tensor]) -> Tensor:
    """``relu(bn(z) + bn_r(r))``; ``par`` / ``rpar``: (scale, shift, ...) rows of one BatchNorm group, or None for the identity."""
    a = torch.empty_like(z)
    pixels, Cp = z.numel() // z.shape[-1], z.shape[-1]
    sc, sh = (None, None) if par is None else (par[0], par[1])
    rs, rh = (None, None) if rpar is None else (rpar[0], rpar[1])
    ops._timed_hbm("bn_add_relu", 6.0 * z.numel(),
                   lambda: L.check(ops._k(z).uclstm_bn_add_relu(_p(z), _p(sc), _p(sh), _p(r), _p(rs), _p(rh), _p(a), pixels, Cp, _stream()),
                                   "bn_add_relu"))
    return a


class Upsample2(torch.autograd.Function):
    """Nearest x2 on 16-bit NHWC; the gradient adds the four children in scan order (a pure function of its input)."""

    @staticmethod
    def forward(ctx, a):
        ops._dev(a, ops.ACT, "activation")
        N, H, W, Cp = a.shape
        out = torch.empty((N, 2 * H, 2 * W, Cp), dtype=a.dtype, device=a.device)
        ops._timed_hbm("upsample2_fwd", 2.0 * (a.numel() + out.numel()),
                       lambda: L.check(ops._k(a).uclstm_upsample2_fwd(_p(a), _p(out), N, H, W, Cp, _stream()), "upsample2_fwd"))
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, H2, W2, Cp = g.shape
        da = torch.empty((N, H2 // 2, W2 // 2, Cp), dtype=g.dtype, device=g.device)
        ops._timed_hbm("upsample2_bwd", 2.0 * (g.numel() + da.numel()),
                       lambda: L.check(ops._k(g).uclstm_upsample2_bwd(_p(g), _p(da), N, H2 // 2, W2 // 2, Cp, _stream()), "upsample2_bwd"))
        return da


class Head3x3(ops._GradAwareFunction):
    """The segmentation head: 16-bit NHWC in, conv3x3 with bias accumulated in f32, f32 NCHW out (never rounded to 16 bits)."""

    @staticmethod
    def forward(ctx, a, weight, bias):
        ops._dev(a, ops.ACT, "activation")
        N, H, W, Cp = a.shape
        Co, Ci = weight.shape[0], weight.shape[1]
        y = torch.empty((N, Co, H, W), dtype=F32, device=a.device)
        ops._timed_hbm("head3x3_fwd", 2.0 * a.numel() + 4.0 * y.numel(),
                       lambda: L.check(ops._k(a).uclstm_head3x3_fwd(_p(a), _p(weight), _p(bias), _p(y), N, H, W, Cp, Ci, Co, _stream()),
                                       "head3x3_fwd"))
        ctx.save_for_backward(a, weight, bias)
        ctx.has_bias = bias is not None
        if ops._will_backward(ctx):
            ops.note_use(weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, weight, _ = ctx.saved_tensors
        N, H, W, Cp = a.shape
        return ops.head_backward(ctx, dy, "head3x3_bwd", ops._k(a).uclstm_head3x3_bwd, L.lib.uclstm_head3x3_bwd_ordered,
                                 (N, H, W, Cp, weight.shape[1], weight.shape[0]), lambda: L.lib.uclstm_head3x3_bwd_ordered_rows(N, H, W),
                                 timed=True)


# ---------------------------------------------------------------------------------------------
# backward of the encoder (csrc/resnet_bwd.hip and the strided descriptors of the GEMM families)
# ---------------------------------------------------------------------------------------------
def maxpool3s2_bwd(a: Tensor, dp: Tensor, dskip: Optional[Tensor]) -> Tensor:
    """Gradient of ``a`` from the gradient ``dp`` of ``maxpool3s2(a)`` plus ``dskip`` (or None), the gradient of its other use."""
    N, H, W, Cp = a.shape
    da = torch.empty_like(a)
    dp = dp.contiguous()
    dskip = None if dskip is None else dskip.contiguous()
    ops._timed_hbm("maxpool3s2_bwd", 2.0 * (a.numel() * (3 if dskip is not None else 2) + dp.numel()),
                   lambda: L.check(ops._k(a).uclstm_maxpool3s2_bwd(_p(a), _p(dp), _p(dskip), _p(da), N, H, W, Cp, _stream()), "maxpool3s2_bwd"))
    return da


class MaxPool3s2(torch.autograd.Function):
    """MaxPool2d(3, 2, 1) of ``a`` plus ``a`` itself as a second output (the skip ConvLSTM's input): the two gradients of the
    stem's activation are added inside the pooling backward kernel (ops.MaxPool2Skip does the same for the UNet)."""

    @staticmethod
    def forward(ctx, a):
        ctx.save_for_backward(a)
        return maxpool3s2(a), a.view_as(a)

    @staticmethod
    def backward(ctx, dp, dskip):
        return dskip if dp is None else maxpool3s2_bwd(ctx.saved_tensors[0], dp, dskip)


# taps of conv3x3 / stride 2 / pad 1 that reach input parity p from the output row j + t: input row 2j + p = 2(j + t) + k - 1
_S2_TAP = ((1, None), (2, 0))          # [p][t] -> k (None: no such tap)
_S2_INDEX: dict = {}                   # device -> the 16 (py, px, ty, tx) -> tap indices (9 = the zero tap), uploaded once


def s2_dgrad_weight(w: Tensor, w_ds: Optional[Tensor] = None) -> Tensor:
    """Weight of the input gradient of conv3x3 / stride 2 / pad 1 as four stride-1 problems, f32 ``[Co, Ci, py, px, ty, tx]``: the
    input pixel (2j + py, 2i + px) reads ``dz`` at (j + ty, i + tx) through ``w[co, ci, ky, kx]`` with ky = 1 for py = 0 (ty = 0 only)
    and ky = 2, 0 for py = 1 (ty = 0, 1); unused taps are zero.  ``w_ds`` (the block's conv1x1 / stride 2, ``[Co, Ci, 1, 1]``) is
    appended along dim 0 as a second source that reaches parity (0, 0) through tap (0, 0) only.  9 tap products per 4 pixels."""
    Co, Ci = w.shape[0], w.shape[1]
    idx = _S2_INDEX.get(w.device)
    if idx is None:
        idx = _S2_INDEX[w.device] = torch.tensor(
            [9 if (_S2_TAP[py][ty] is None or _S2_TAP[px][tx] is None) else _S2_TAP[py][ty] * 3 + _S2_TAP[px][tx]
             for py in (0, 1) for px in (0, 1) for ty in (0, 1) for tx in (0, 1)], device=w.device)
    wz = torch.nn.functional.pad(w.reshape(Co, Ci, 9), (0, 1))                    # column 9: the zero tap
    out = wz[:, :, idx]
    if w_ds is not None:
        ds = torch.nn.functional.pad(w_ds.reshape(w_ds.shape[0], Ci, 1), (0, 15))          # (py, px, ty, tx) = 0 only
        out = torch.cat([out, ds], 0)
    return out.reshape(-1, Ci, 2, 2, 2, 2).contiguous()


def s2_dgrad_pack_desc(Ci: int, Co: int, nsrc: int) -> L.PackDesc:
    """Panel of ``s2_dgrad_weight``: rows (parity, ci) -- four segments of cpad(Ci) rows -- and K = (tap (ty, tx), source, co)."""
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = 4 * cpad(Ci), 4, nsrc
    d.kseg[0], d.kseg[1] = kseg(cpad(Co)), (kseg(cpad(Co)) if nsrc > 1 else 0)
    d.cvalid[0], d.cvalid[1] = Co, (Co if nsrc > 1 else 0)
    d.choff[0], d.choff[1] = 0, Co
    d.Ktot = 4 * (d.kseg[0] + d.kseg[1])
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_TAPMAJOR, Ci, cpad(Ci)
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = 16, Ci * 16, 1, 4
    return d


def conv_s2_dgrad(dz: Tensor, weight: Tensor, dz_ds: Optional[Tensor] = None, w_ds: Optional[Tensor] = None) -> Tensor:
    """Input gradient of conv3x3 / stride 2 / pad 1 (plus, folded in as a second source of the same launch, that of the conv1x1 /
    stride 2 of the same input): ONE forward-family launch with ktap 2 on the Ho x Wo grid of ``dz`` and four output segments with
    scale 2, oy = py, ox = px (the layout ConvT2x2 writes forward).  The input is (2 Ho, 2 Wo): even sizes only."""
    n, Ho, Wo, _ = dz.shape
    Co, Ci = weight.shape[0], weight.shape[1]
    nsrc = 1 if dz_ds is None else 2
    dd = s2_dgrad_pack_desc(Ci, Co, nsrc)
    # the rearranged weight is a temporary: packed in line, never by the look-ahead plan
    wd = ops.pack_weights(dd, s2_dgrad_weight(weight, w_ds if nsrc > 1 else None), 0, dz.dtype, lookahead=False)
    Cip = cpad(Ci)
    dx = torch.empty((n, 2 * Ho, 2 * Wo, Cip), dtype=dz.dtype, device=dz.device)
    segs = [(dx, t * Cip, (t + 1) * Cip, 0, 2, t // 2, t % 2) for t in range(4)]
    srcs = [SrcView(dz)] + ([SrcView(dz_ds)] if nsrc > 1 else [])
    ops.igemm_store(srcs, wd, (Ho, Wo), n, segs, ktap=2, pad=0)
    return dx


def _bn_args(bn: nn.BatchNorm2d, pending: list):
    """``bn`` as the kernels take it, for one use in a forward pass: (gamma, beta, running mean, running variance, uses batch
    statistics, momentum argument, eps).  In training mode its counter goes to ``pending`` (one multi-tensor add per forward).
    Plain tuples here and in conv_geometry: the eager frame-by-frame path is host-bound."""
    training, mom = bn_mode(bn, bn.training)
    if training and bn.num_batches_tracked is not None:
        pending.append((bn.num_batches_tracked, 1))
    return bn.weight, bn.bias, bn.running_mean, bn.running_var, training, mom, bn.eps


def _conv_bn_forward(x: Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, stride: int, pending: list, relu: bool, im2col: bool):
    """A bias-free convolution of the encoder that is not under autograd, on the bodies of ops.py (``im2col``: ``x`` is the
    pre-gathered 7x7 stem matrix): (z, par), or (the finished activation, None) where BatchNorm (and ReLU if ``relu``) went into the
    GEMM's epilogue -- exactly when this BatchNorm uses its running statistics."""
    w, args = conv.weight, _bn_args(bn, pending)
    geom = ops.conv_geometry(x, None, w, (w.shape[1],), (0, 0), im2col7_pack_desc if im2col else None, stride)
    if args[4]:
        return ops.conv_bn_stats(x, w, None, geom, args)[:2]
    return ops.conv_bn_fold(x, w, None, geom, args, relu), None


class EncConv(ops._GradAwareFunction):
    """A bias-free convolution of the trainable encoder and its BatchNorm constants: ``(z, par, z_ds, par_ds)``, ``z`` the
    pre-BatchNorm output.  ``w_ds``: the conv1x1 / stride 2 of the same input (a strided BasicBlock), so that the block's input
    gradient is ONE launch (conv_s2_dgrad).  ``im2col``: ``x`` is the pre-gathered 7x7 stem matrix, which gets no gradient.
    Forward and backward on the bodies of ops.py (ops.conv_bn_stats, ops.conv_wgrad -- weight gradients over the OUTPUT grid:
    ktap k, scale = stride -- and ops.conv3x3_dgrad).  The ``sync`` marker of conv_bn_stats is dropped here and BnRelu / BnAddRelu
    differentiate with this rank's sums: sync_batchnorm is not supported with a trainable encoder."""

    @staticmethod
    def _geometry(x, w, stride, im2col):
        return ops.conv_geometry(x, None, w, (w.shape[1],), (0, 0), im2col7_pack_desc if im2col else None, stride)

    @staticmethod
    def forward(ctx, x, weight, w_ds, bn, bn_ds, stride, im2col):
        ops._dev(x, ops.ACT, "activation")
        if stride == 2 and not im2col and (x.shape[1] % 2 or x.shape[2] % 2):          # conv_s2_dgrad writes a (2 Ho, 2 Wo) input
            raise UclstmError("EncConv: a stride-2 convolution with a backward pass needs even input sizes")
        z, par, _ = ops.conv_bn_stats(x, weight, None, EncConv._geometry(x, weight, stride, im2col), bn)
        z_ds = par_ds = None
        if w_ds is not None:
            z_ds, par_ds, _ = ops.conv_bn_stats(x, w_ds, None, EncConv._geometry(x, w_ds, stride, False), bn_ds)
        ctx.mark_non_differentiable(*[t for t in (par, par_ds) if t is not None])
        ctx.save_for_backward(x, weight, w_ds)
        ctx.cfg = (stride, im2col)
        if ops._will_backward(ctx):
            ops.note_use(weight, w_ds)
        return z, par, z_ds, par_ds

    @staticmethod
    def backward(ctx, dz, _dpar, dz_ds, _dpar_ds):
        x, weight, w_ds = ctx.saved_tensors
        stride, im2col = ctx.cfg
        dz = dz.contiguous()
        dz_ds = None if (dz_ds is None or w_ds is None) else dz_ds.contiguous()
        dweight = dw_ds = dx = None
        if ctx.needs_input_grad[1]:
            dweight = ops.conv_wgrad(weight, EncConv._geometry(x, weight, stride, im2col), dz)
        if dz_ds is not None and ctx.needs_input_grad[2]:
            dw_ds = ops.conv_wgrad(w_ds, EncConv._geometry(x, w_ds, stride, False), dz_ds)
        if ctx.needs_input_grad[0] and not im2col:
            dx = conv_s2_dgrad(dz, weight, dz_ds, w_ds) if stride == 2 else ops.conv3x3_dgrad(dz, weight, x, weight.shape[1])
        return dx, dweight, dw_ds, None, None, None, None


class BnRelu(ops._GradAwareFunction):
    """``relu(z*scale + shift)`` with the constants ``par`` of EncConv; backward with uclstm_bn_bwd_reduce / _apply as one group.
    ``training`` False: evaluation statistics with a backward pass (zero sums in the apply pass: dz = scale*g)."""

    @staticmethod
    def forward(ctx, z, par, gamma, beta, training):
        a = ops.bn_relu(z, par)
        ctx.save_for_backward(z, par, gamma, beta)
        ctx.training = training
        if ops._will_backward(ctx):
            ops.note_use(gamma, beta)
        return a

    @staticmethod
    def backward(ctx, da):
        z, par, gamma, beta = ctx.saved_tensors
        need_z, _, need_gamma, need_beta, _ = ctx.needs_input_grad
        # ops.bn_relu_backward, one kernel per call: no reduction where the statistics are frozen and neither gamma nor beta wants a
        # gradient, the parameter gradients launched between the two kernels, no apply pass where z needs no gradient
        sums = dz = None
        if ctx.training or need_gamma or need_beta:
            _, sums = ops.bn_relu_backward(z, par, da, 1, ctx.training, None, want_dz=False)
        dgamma, dbeta, _ = ops.bn_param_grads(need_gamma, need_beta, gamma, beta, sums, gamma.shape[0])
        if need_z:
            dz, _ = ops.bn_relu_backward(z, par, da, 1, ctx.training, None, want_sums=False, sums=sums)
        return dz, None, dgamma, dbeta, None


class BnAddRelu(ops._GradAwareFunction):
    """Tail of a BasicBlock, ``relu(bn(z) + bn_r(r))`` (``rpar`` None: ``r`` is the block's input as it is).  Backward with
    uclstm_bn_add_relu_bwd_reduce / _apply: the sums of both BatchNorms from one pass over (z, r, da), then dz and dr from a
    second; a branch nobody needs is not written.  ``training`` / ``rtraining`` False: evaluation statistics, per branch."""

    @staticmethod
    def forward(ctx, z, par, gamma, beta, r, rpar, rgamma, rbeta, training, rtraining):
        a = bn_add_relu(z, par, r, rpar)
        ctx.save_for_backward(z, par, gamma, beta, r, rpar, rgamma, rbeta)
        ctx.training, ctx.rtraining = training, rtraining
        if ops._will_backward(ctx):
            ops.note_use(gamma, beta, rgamma, rbeta)
        return a

    @staticmethod
    def backward(ctx, da):
        z, par, gamma, beta, r, rpar, rgamma, rbeta = ctx.saved_tensors
        need = ctx.needs_input_grad
        pixels, Cp, dev = z.numel() // z.shape[-1], z.shape[-1], z.device
        K, da = ops._k(z), da.contiguous()
        raff = rpar is not None
        pq = (_p(par[0]), _p(par[1]), _p(par[2]), _p(par[3]))
        rq = (_p(rpar[0]), _p(rpar[1]), _p(rpar[2]), _p(rpar[3])) if raff else (None, None, None, None)
        zero = None
        sums = torch.empty((1, Cp, 2), dtype=F32, device=dev)
        rsums = torch.empty((1, Cp, 2), dtype=F32, device=dev) if raff else None
        need_reduce = (ctx.training and need[0]) or need[2] or need[3] or (raff and ((ctx.rtraining and need[4]) or need[6] or need[7]))
        if need_reduce:
            partials = torch.empty((int(L.lib.uclstm_bn_add_relu_bwd_rows(pixels)), Cp, 3), dtype=F32, device=dev)
            ops._timed_hbm("bn_add_relu_bwd_reduce", 6.0 * z.numel(),
                           lambda: L.check(K.uclstm_bn_add_relu_bwd_reduce(_p(z), *pq, _p(r), *rq, _p(da), _p(partials), _p(sums), _p(rsums),
                                                                           pixels, Cp, _stream()), "bn_add_relu_bwd_reduce"))
        dgamma, dbeta, _ = ops.bn_param_grads(need[2], need[3], gamma, beta, sums, gamma.shape[0])
        drgamma = drbeta = None
        if raff:
            drgamma, drbeta, _ = ops.bn_param_grads(need[6], need[7], rgamma, rbeta, rsums, rgamma.shape[0])
        dz = dr = None
        if need[0] or need[4]:
            if not (ctx.training and need_reduce) or (raff and not ctx.rtraining):
                zero = torch.zeros((1, Cp, 2), dtype=F32, device=dev)
            s_z = sums if (ctx.training and need_reduce) else zero
            s_r = None if not raff else (rsums if (ctx.rtraining and need_reduce) else zero)
            dz = torch.empty_like(z) if need[0] else None
            dr = torch.empty_like(r) if need[4] else None
            nb = 2.0 * z.numel() * (3 + (dz is not None) + (dr is not None))
            ops._timed_hbm("bn_add_relu_bwd_apply", nb,
                           lambda: L.check(K.uclstm_bn_add_relu_bwd_apply(_p(z), *pq, _p(s_z), _p(r), *rq, _p(s_r), _p(da), _p(dz), _p(dr),
                                                                          pixels, Cp, _stream()), "bn_add_relu_bwd_apply"))
        return dz, None, dgamma, dbeta, dr, None, drgamma, drbeta, None, None


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
class PretrainedTemporalUNet(nn.Module):
    """Reference train/resnet18.py:19-139.

    ``model(x_seq[B,T,2,H,W] f32) -> (y[B,T,out_channels,H,W] f32, None)``; H and W multiples of 32.

    ``encoder_weights``: ``None`` (random: ``kaiming_normal_(mode="fan_out")`` convolutions, BatchNorm weight 1 / bias 0), a
    torchvision-layout ResNet18 ``state_dict`` or a path to one (``fc.*`` ignored, a 3-channel ``conv1.weight`` adapted to two
    channels as smp does: ``w[:, :2] * 1.5``).  Nothing is ever downloaded: pretrained weights come from that file or from the
    checkpoint loaded afterwards.

    Where this differs from running the reference's code line by line:

    * ``lstm_skips[0]`` works on the raw input, a feature smp's decoder drops: the reference computes it and throws it away.
      Here it is not computed, and its parameters have ``requires_grad=False`` -- in the reference their ``.grad`` stays ``None``
      and ``torch.optim.AdamW`` skips them; ``FusedAdamW(filter(requires_grad))`` leaves them out the same way.
    * A frozen encoder runs without autograd: no backward kernel is launched for it, and none for the input half of the skip
      ConvLSTMs' gate convolutions.  ``freeze_encoder`` only sets ``requires_grad=False``: after ``model.train()`` the frozen
      encoder still normalises with batch statistics and updates its running statistics, as the reference does.
    * Training the encoder is opt-in: ``model.unfreeze_encoder(stages)`` (see there).  Without it, ``freeze_encoder=False``
      constructs, loads and runs under ``torch.no_grad()``, and a forward in grad mode while an encoder parameter requires grad
      raises ``UclstmError`` naming that method.
    * BatchNorm statistics are those of the whole ``B*T`` batch (one group), in the encoder and in the decoder.
    """

    def __init__(self, out_channels: int = 1, lstm_layers: int = 1, freeze_encoder: bool = True, encoder_weights=None):
        super().__init__()
        if not 1 <= out_channels <= HEAD_MAX_OUT:
            raise UclstmError(f"PretrainedTemporalUNet: out_channels must be 1..{HEAD_MAX_OUT} (the 3x3 head kernel keeps them in registers)")
        self.base_model = _BaseModel(out_channels)
        self.encoder = self.base_model.encoder
        self.decoder = self.base_model.decoder
        self.head = self.base_model.segmentation_head
        for m in self.base_model.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        if encoder_weights is not None:
            self.load_encoder_weights(encoder_weights)
        if freeze_encoder:
            for p in self.encoder.parameters():
                p.requires_grad = False
        self.lstm_input_dim = ENCODER_CHANNELS[-1]
        self.lstm = ConvLSTM(self.lstm_input_dim, self.lstm_input_dim, num_layers=lstm_layers, kernel_size=3)
        self.skip_channels = list(ENCODER_CHANNELS[:-1])
        self.lstm_skips = nn.ModuleList(ConvLSTM(ch, ch, num_layers=lstm_layers, kernel_size=3) for ch in self.skip_channels)
        self.lstm_skips[0].requires_grad_(False)          # never computed: see the class docstring
        self.out_channels = out_channels
        self._encoder_opt_in = False                       # unfreeze_encoder(): see there

    def load_encoder_weights(self, weights) -> None:
        """``weights``: a torchvision-layout ResNet18 state_dict or a path to one."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu")
        sd = {k: v for k, v in weights.items() if not k.startswith("fc.")}
        sd["conv1.weight"] = adapt_first_conv(sd["conv1.weight"])
        self.encoder.load_state_dict(sd, strict=True)

    def encoder_stage(self, name: str) -> list:
        """The modules of one encoder stage: ``"stem"`` (conv1, bn1), ``"layer1"`` .. ``"layer4"``."""
        if name not in ENCODER_STAGES:
            raise UclstmError(f"PretrainedTemporalUNet: unknown encoder stage {name!r} (stages: {', '.join(ENCODER_STAGES)})")
        enc = self.encoder
        return [enc.conv1, enc.bn1] if name == "stem" else [getattr(enc, name)]

    def unfreeze_encoder(self, stages="all") -> "PretrainedTemporalUNet":
        """Opt in to training the encoder: ``requires_grad=True`` on the parameters of the named stages (``"all"``, one name or a
        sequence of ``"stem"``, ``"layer1"`` .. ``"layer4"``), ``False`` on every other encoder parameter; ``()`` freezes the
        whole encoder again.  From then on each parameter's own ``requires_grad`` decides what is computed (weight, gamma and
        beta independently, so single parameters may be toggled afterwards): stages below the lowest one with a trainable
        parameter run without autograd exactly as in the frozen model, the others keep their activations and run the backward
        kernels of csrc/resnet_bwd.hip and the strided input- / weight-gradient descriptors.  BatchNorm mode stays per module:
        after ``model.train(); model.encoder.eval()`` the weights train against frozen statistics."""
        names = ENCODER_STAGES if stages == "all" else ((stages,) if isinstance(stages, str) else tuple(stages))
        chosen = {id(p) for n in names for m in self.encoder_stage(n) for p in m.parameters()}
        for p in self.encoder.parameters():
            p.requires_grad = id(p) in chosen
        self._encoder_opt_in = True
        return self

    def _first_trainable_stage(self) -> Optional[int]:
        """Index into ENCODER_STAGES of the lowest stage with a parameter that requires grad (None: the encoder is frozen)."""
        for i, name in enumerate(ENCODER_STAGES):
            if any(p.requires_grad for m in self.encoder_stage(name) for p in m.parameters()):
                return i
        return None

    # -- encoder: ONE route.  ``grad``: the stage runs under autograd (EncConv, BnRelu, BnAddRelu, MaxPool3s2); without it the plain
    #    functions those Functions call run directly, under no_grad -- the forward-only route pays for no Function.apply ----------
    @staticmethod
    def _conv_bn(x: Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, ds: Optional[nn.Sequential], pending: list, grad: bool,
                 relu: bool = False, im2col: bool = False):
        """``(z, par, z_ds, par_ds)`` of ``conv`` and (``ds``: the block's downsample pair) of the conv1x1 of the same input, launched
        right behind it.  ``par`` None: ``z`` is finished (the fold: that BatchNorm uses its running statistics and the stage is
        not under autograd)."""
        stride = conv.stride[0]
        if grad:
            return EncConv.apply(x, conv.weight, None if ds is None else ds[0].weight, _bn_args(bn, pending),
                                 None if ds is None else _bn_args(ds[1], pending), stride, im2col)
        main = _conv_bn_forward(x, conv, bn, stride, pending, relu, im2col)
        return main + ((None, None) if ds is None else _conv_bn_forward(x, ds[0], ds[1], stride, pending, False, False))

    @staticmethod
    def _bn_relu(z: Tensor, par: Optional[Tensor], bn: nn.BatchNorm2d, grad: bool) -> Tensor:
        if par is None:
            return z
        return BnRelu.apply(z, par, bn.weight, bn.bias, bn_mode(bn, bn.training)[0]) if grad else ops.bn_relu(z, par)

    def _block(self, x: Tensor, blk: BasicBlock, pending: list, grad: bool) -> Tensor:
        ds = blk.downsample
        z1, par1, r, rpar = self._conv_bn(x, blk.conv1, blk.bn1, ds, pending, grad, relu=True)
        a1 = self._bn_relu(z1, par1, blk.bn1, grad)
        z2, par2, _, _ = self._conv_bn(a1, blk.conv2, blk.bn2, None, pending, grad)
        if ds is None:
            r = x
        if not grad:
            return bn_add_relu(z2, par2, r, rpar)
        rbn = (None, None, False) if ds is None else (ds[1].weight, ds[1].bias, bn_mode(ds[1], ds[1].training)[0])
        return BnAddRelu.apply(z2, par2, blk.bn2.weight, blk.bn2.bias, r, rpar, rbn[0], rbn[1], bn_mode(blk.bn2, blk.bn2.training)[0], rbn[2])

    def _encode(self, x_seq: Tensor, pending: list, first: Optional[int] = None):
        """f32 [B,T,2,H,W] -> (f1 .. f5), 16-bit NHWC with image ``t*B + b``, at H/2 .. H/32.  ``first``: index into ENCODER_STAGES
        of the lowest stage under autograd; None: none, and the caller runs this under no_grad.  The stem never computes an input
        gradient."""
        enc, feats = self.encoder, []

        def stage(i: int, a: Tensor) -> Tensor:
            grad = first is not None and i >= first
            if i == 0:
                z, par, _, _ = self._conv_bn(a, enc.conv1, enc.bn1, None, pending, grad, relu=True, im2col=True)
                f1 = self._bn_relu(z, par, enc.bn1, grad)
                a, f1 = MaxPool3s2.apply(f1) if grad else (maxpool3s2(f1), f1)
                feats.append(f1)
                return a
            for blk in getattr(enc, ENCODER_STAGES[i]):
                a = self._block(a, blk, pending, grad)
            feats.append(a)
            return a

        a = im2col7x7s2_first(x_seq)
        for i in range(len(ENCODER_STAGES)):
            if first is None or i >= first:
                a = stage(i, a)
            else:
                with torch.no_grad():          # below the lowest trainable stage: as in the frozen model
                    a = stage(i, a)
        return feats

    # -- decoder --------------------------------------------------------------------------------
    @staticmethod
    def _stage(seq: nn.Sequential, x0: Tensor, x1: Optional[Tensor], c_valid, pending: list) -> Tensor:
        gamma, beta, rm, rv, training, mom, eps = _bn_args(seq[1], pending)
        return ops.ConvBNReLU.apply(x0, x1, seq[0].weight, None, gamma, beta, rm, rv, tuple(c_valid), (0, 0), 1, training, mom, eps, False)

    def _decoder_block(self, blk: DecoderBlock, x: Tensor, skip: Optional[Tensor], pending: list) -> Tensor:
        """One DecoderBlock: ``x`` [n, h, w, cin] and ``skip`` [n, 2h, 2w, cskip] (None: the last block) -> [n, 2h, 2w, cout]."""
        cin, cskip, cout = blk.channels
        up = Upsample2.apply(x)
        x = self._stage(blk.conv1, up, skip, (cin, cskip) if skip is not None else (cin,), pending)
        return self._stage(blk.conv2, x, None, (cout,), pending)

    def _decode(self, x: Tensor, skips, pending: list) -> Tensor:
        """The five blocks of the decoder on ``x`` (the bottleneck, 16-bit NHWC) and ``skips`` (deepest first, None for the last block),
        then the head: f32 ``[n, out_channels, H, W]``."""
        for blk, skip in zip(self.decoder.blocks, skips):
            x = self._decoder_block(blk, x, skip, pending)
        conv = self.head[0]
        return Head3x3.apply(x, conv.weight, conv.bias)

    @staticmethod
    def _check_input(x: Tensor, who: str, ndim: int) -> None:
        """``ndim`` 5: a sequence [B, T, C, H, W]; 4: one frame [B, C, H, W]."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise UclstmError(f"{who}: a HIP device tensor is required (this package has no CPU path)")
        if x.dim() != ndim or x.shape[-3] != ENCODER_CHANNELS[0]:
            raise UclstmError(f"{who}: expected [B, {'T, ' if ndim == 5 else ''}{ENCODER_CHANNELS[0]}, H, W], got {tuple(x.shape)}")
        H, W = x.shape[-2:]
        if H % 32 or W % 32:
            raise UclstmError(f"{who}: H and W must be multiples of 32 (five stride-2 stages), got {H} x {W}")

    def forward(self, x_seq: Tensor):
        self._check_input(x_seq, "PretrainedTemporalUNet", 5)
        if torch.is_grad_enabled() and not self._encoder_opt_in and any(p.requires_grad for p in self.encoder.parameters()):
            raise UclstmError("PretrainedTemporalUNet: training an unfrozen encoder is opt-in: call model.unfreeze_encoder() (all "
                              "stages, or e.g. (\"layer3\", \"layer4\")) first, construct with freeze_encoder=True, or run under "
                              "torch.no_grad()")
        pending: list = []
        try:
            return self._forward(x_seq.contiguous().float(), pending), None
        finally:
            if pending:
                modules._flush_counters(pending)
            ops.join_forward_side(x_seq.device)          # BatchNorm running statistics were updated on the second stream

    # -- streaming: one frame in, one frame out, all five recurrent states carried ------------------
    STATE_KEYS = ("lstm", "skip1", "skip2", "skip3", "skip4")

    def _recurrences(self):
        """(state key, ConvLSTM, index of its encoder feature) of the five computed recurrences, ``lstm`` first."""
        return [("lstm", self.lstm, 4)] + [(f"skip{j}", self.lstm_skips[j], j - 1) for j in (1, 2, 3, 4)]

    def state_spec(self, B: int, H: int, W: int) -> dict:
        """``{key: (layers, (B, h, w, padded channels))}``: the shapes of the recurrent state ``step_nhwc`` carries."""
        return {key: (len(lstm.layers), (B, H >> (fi + 1), W >> (fi + 1), cpad(lstm.layers[0].hidden_dim)))
                for key, lstm, fi in self._recurrences()}

    def step_nhwc(self, x_t: Tensor, full_state: Optional[dict] = None, out_state: Optional[dict] = None):
        """``x_t`` f32 ``[B, 2, H, W]`` -> ``(y_t f32 [B, out_channels, H, W], new_state)``: one frame of ``forward()``.

        ``full_state`` maps ``'lstm'`` and ``'skip1'`` .. ``'skip4'`` (``lstm_skips[1..4]``; ``lstm_skips[0]`` is never computed)
        to per-layer lists of ``(h 16-bit NHWC, c f32 NHWC)``; ``None`` is the zero state.  Feeding frames one by one reproduces
        ``forward()`` on the whole sequence in evaluation mode.  ``out_state`` (same structure): the buffers the new state is
        written into -- no copies; h buffers must differ from the input state's, c buffers may be the same tensors.

        One step: the encoder on the frame, layer l of all five ConvLSTMs as ONE ``ops.convlstm_tick`` (l = 0, 1, ...), the
        decoder, the head.  Inference only: it raises in grad mode, and while any BatchNorm is in training mode (a one-frame
        batch statistic is not what ``forward`` computes, and it would move the running statistics)."""
        self._check_input(x_t, "PretrainedTemporalUNet.step_nhwc", 4)
        B, _, H, W = x_t.shape
        if torch.is_grad_enabled():
            raise UclstmError("PretrainedTemporalUNet.step_nhwc is inference only: call it under torch.no_grad()")
        if any(isinstance(m, nn.BatchNorm2d) and bn_mode(m, m.training)[0] for m in self.modules()):
            raise UclstmError("PretrainedTemporalUNet.step_nhwc: a BatchNorm is in training mode (batch statistics of one frame are "
                              "not what forward() computes): call model.eval() first")
        adt, dev = ops.get_compute_dtype(), x_t.device
        spec = self.state_spec(B, H, W)
        st = {} if full_state is None else full_state
        ost = {} if out_state is None else out_state
        cur, new_state = {}, {}
        for key, (n_layers, shape) in spec.items():
            cur[key] = st.get(key) or [(torch.zeros(shape, dtype=adt, device=dev), torch.zeros(shape, dtype=F32, device=dev))
                                       for _ in range(n_layers)]
            new_state[key] = ost.get(key) or [(torch.empty(shape, dtype=adt, device=dev), torch.empty(shape, dtype=F32, device=dev))
                                              for _ in range(n_layers)]
            if len(cur[key]) != n_layers or len(new_state[key]) != n_layers:
                raise UclstmError(f"PretrainedTemporalUNet.step_nhwc: state {key!r} must hold one (h, c) per layer ({n_layers})")
        pending: list = []
        feats = self._encode(x_t.contiguous().float().unsqueeze(1), pending)
        recs = self._recurrences()
        xs = {key: feats[fi] for key, _, fi in recs}
        for li in range(len(self.lstm.layers)):
            members = []
            for key, lstm, _ in recs:
                cell = lstm.layers[li]
                (h_prev, c_prev), (h_out, c_out) = cur[key][li], new_state[key][li]
                members.append((xs[key], h_prev, c_prev, h_out, c_out, cell.conv.weight, cell.conv.bias, cell.hidden_dim, cell.input_dim))
                xs[key] = h_out
            ops.convlstm_tick(members)
        ops.join_forward_side(dev)          # (nothing is pending here: every evaluation-mode stage above has joined already)
        return self._decode(xs["lstm"], [xs[f"skip{j}"] for j in (4, 3, 2, 1)] + [None], pending), new_state

    def _forward(self, x_seq: Tensor, pending: list) -> Tensor:
        B, T, _, H, W = x_seq.shape
        first = self._first_trainable_stage() if (torch.is_grad_enabled() and self._encoder_opt_in) else None
        with torch.set_grad_enabled(first is not None):
            feats = self._encode(x_seq, pending, first)

        def run(lstm: ConvLSTM, f: Tensor) -> Tensor:          # [T*B,h,w,C] -> the last layer's h for all steps, same shape
            out, _ = lstm.seq_nhwc(f.view(T, B, *f.shape[1:]), None)
            return out.reshape(T * B, *out.shape[2:])

        x = run(self.lstm, feats[4])
        y = self._decode(x, [run(self.lstm_skips[j], feats[j - 1]) for j in (4, 3, 2, 1)] + [None], pending)
        return y.view(T, B, self.out_channels, H, W).transpose(0, 1)
