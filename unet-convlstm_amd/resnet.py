"""The reference's shipped model, train/resnet18.py: a ResNet18 encoder, five ConvLSTMs and smp's UNet decoder, on libuclstm.so.

``PretrainedTemporalUNet`` keeps the reference's constructor, attribute names and ``state_dict`` keys (those of
``smp.Unet("resnet18", in_channels=2, decoder_channels=(256, 128, 64, 32, 16))`` registered twice, as
``train/resnet18.py:26-38`` does, plus ``lstm`` and ``lstm_skips``), so a ``resnet18_frozen_*`` checkpoint loads with
``strict=True``.  Neither ``segmentation_models_pytorch`` nor ``torchvision`` is imported: the containers are stock
``nn.Conv2d`` / ``nn.BatchNorm2d`` modules that are never called, and every forward goes through HIP kernels -- the
implicit-GEMM family for the convolutions (stride 2 is a descriptor with ``scale = 2``), ``ops.ConvBNReLU`` for the decoder
stages, this package's ``ConvLSTM`` for the recurrences and the kernels of ``csrc/resnet.hip`` around them.

Not part of this module: training an unfrozen encoder (there is no strided input-gradient or weight-gradient GEMM),
``GraphedTrainStep``, ``StreamingPredictor`` and ``sync_batchnorm`` with this model, and a fused upsample.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import modules, ops
from ._lib import UclstmError
from .modules import ConvLSTM
from .ops import F32, SrcView, _p, _stream, cpad, kseg

Tensor = torch.Tensor

ENCODER_CHANNELS = (2, 64, 64, 128, 256, 512)          # smp's resnet18 encoder.out_channels with in_channels = 2
DECODER_CHANNELS = (256, 128, 64, 32, 16)              # train/resnet18.py:32
HEAD_MAX_OUT = 4                                       # uclstm_head3x3_*: output channels are register accumulators

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
def conv_desc(Co: int, Ci: int, k: int, c_pad: int) -> L.PackDesc:
    """Forward panel of a k x k convolution over one source (ops.conv_pack_desc for any tap count)."""
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = cpad(Co), k * k, 1
    d.kseg[0], d.kseg[1] = kseg(c_pad), 0
    d.cvalid[0], d.cvalid[1] = Ci, 0
    d.choff[0] = d.choff[1] = 0
    d.Ktot = k * k * d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, Co, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = Ci * k * k, k * k, 1, 0
    return d


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
        a, weight, bias = ctx.saved_tensors
        dy = dy.contiguous().float()
        N, H, W, Cp = a.shape
        Co, Ci = weight.shape[0], weight.shape[1]
        dev = a.device
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        geom = (N, H, W, Cp, Ci, Co)
        if not (need_w or need_b):
            if da is not None:
                L.check(ops._k(a).uclstm_head3x3_bwd(_p(a), _p(weight), _p(dy), _p(da), None, None, *geom, _stream()), "head3x3_bwd")
            return da, None, None
        # the kernels ADD into dw / db: with attached f32 gradients straight into them, as ops.OutConv1x1
        direct = ops.direct_grad_pair(weight, bias, need_w, need_b)
        gw, gb = direct or (None, None)
        nbytes = 2.0 * a.numel() * (2 if da is not None else 1) + 4.0 * dy.numel()
        if ops.is_deterministic():
            dw = gw if direct else (torch.empty_like(weight, memory_format=torch.contiguous_format) if need_w else None)
            db = gb if (direct and ctx.has_bias) else (torch.empty((Co,), dtype=F32, device=dev) if need_b else None)
            rows = int(L.lib.uclstm_head3x3_bwd_ordered_rows(N, H, W))
            partials = torch.empty((rows * (Co * Ci * 9 + Co),), dtype=F32, device=dev)
            ops._log_reduce("head3x3_bwd_ordered")
            ops._timed_hbm("head3x3_bwd", nbytes,
                           lambda: L.check(L.lib.uclstm_head3x3_bwd_ordered(_p(a), _p(weight), _p(dy), _p(da), _p(partials), _p(dw), _p(db),
                                                                            1 if direct else 0, *geom, L.act_type(a.dtype), _stream()),
                                           "head3x3_bwd_ordered"))
        else:
            dw = gw if direct else (torch.zeros_like(weight, memory_format=torch.contiguous_format) if need_w else None)
            db = gb if (direct and ctx.has_bias) else (torch.zeros((Co,), dtype=F32, device=dev) if need_b else None)
            ops._log_reduce("head3x3_bwd")
            ops._timed_hbm("head3x3_bwd", nbytes,
                           lambda: L.check(ops._k(a).uclstm_head3x3_bwd(_p(a), _p(weight), _p(dy), _p(da), _p(dw), _p(db), *geom, _stream()),
                                           "head3x3_bwd"))
        if direct:
            ops.grad_written(weight)
            if ctx.has_bias:
                ops.grad_written(bias)
            return da, None, None
        return da, (dw if need_w else None), (db if need_b else None)


def _bn_mode(bn: nn.BatchNorm2d):
    """(uses batch statistics, momentum argument of the BatchNorm kernels) -- the rule of modules.DoubleConv._stage."""
    training = bn.training or not bn.track_running_stats
    if bn.momentum is not None:
        mom = bn.momentum
    elif training and bn.num_batches_tracked is not None:
        mom = -float(int(bn.num_batches_tracked) + 1)
    else:
        mom = 0.0
    return training, mom


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
    * ``freeze_encoder=False`` constructs, loads and runs under ``torch.no_grad()``; a forward in grad mode while an encoder
      parameter requires grad raises ``UclstmError`` (there is no strided input-gradient / weight-gradient GEMM).
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

    def load_encoder_weights(self, weights) -> None:
        """``weights``: a torchvision-layout ResNet18 state_dict or a path to one."""
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu")
        sd = {k: v for k, v in weights.items() if not k.startswith("fc.")}
        sd["conv1.weight"] = adapt_first_conv(sd["conv1.weight"])
        self.encoder.load_state_dict(sd, strict=True)

    # -- encoder: forward-only stages -----------------------------------------------------------
    def _conv_bn(self, x: Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, relu: bool, pending: list, im2col: bool = False):
        """conv (+ BatchNorm statistics).  Training mode: (pre-BatchNorm z, par) -- the caller applies the affine; evaluation
        mode: (BatchNorm folded into the epilogue, with ReLU if ``relu``, None)."""
        n, Hs, Ws, Cxp = x.shape
        Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
        Cop, dev = cpad(Co), x.device
        if im2col:
            k, s, pad, (Ho, Wo) = 1, 1, 0, (Hs, Ws)
            pd = im2col7_pack_desc(Co, Ci, Cxp)
        else:
            k, s = conv.kernel_size[0], conv.stride[0]
            pad, Ho, Wo = k // 2, (Hs - 1) // s + 1, (Ws - 1) // s + 1
            pd = conv_desc(Co, Ci, k, Cxp)
        wp = ops.pack_weights(pd, conv.weight, 0, x.dtype)
        out = torch.empty((n, Ho, Wo, Cop), dtype=x.dtype, device=dev)
        seg = [(out, 0, Cop, 0, 1, 0, 0)]
        training, mom = _bn_mode(bn)
        if not training:
            ops.join_forward_side(dev)
            par = ops._eval_bn_constants(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mom, Co, Cop)
            ops.igemm_store([SrcView(x)], wp, (Ho, Wo), n, seg, ktap=k, scale=s, pad=pad, col_scale=par[0], col_shift=par[1], relu=relu)
            return out, None
        stats = torch.empty((1, L.lib.uclstm_igemm_tiles_per_group(n, Ho, Wo, 1, Cop), Cop, 2), dtype=F32, device=dev)
        ops.igemm_store([SrcView(x)], wp, (Ho, Wo), n, seg, ktap=k, scale=s, pad=pad, groups=1, stats=stats)
        par, _ = ops._bn_forward_stats(stats, n, Ho, Wo, 1, Co, bn.weight, bn.bias, bn.running_mean, bn.running_var, mom, bn.eps, "plain")
        if bn.num_batches_tracked is not None:
            pending.append((bn.num_batches_tracked, 1))
        return out, par

    def _conv_bn_relu(self, x, conv, bn, pending, im2col=False) -> Tensor:
        z, par = self._conv_bn(x, conv, bn, True, pending, im2col)
        if par is None:
            return z
        a = torch.empty_like(z)
        pixels = z.numel() // z.shape[-1]
        ops._timed_hbm("bn_apply_relu", 4.0 * z.numel(),
                       lambda: L.check(ops._k(z).uclstm_bn_apply_relu(_p(z), _p(a), _p(par[0]), _p(par[1]), pixels, pixels, z.shape[-1],
                                                                      _stream()), "bn_apply_relu"))
        return a

    def _block(self, x: Tensor, blk: BasicBlock, pending: list) -> Tensor:
        a1 = self._conv_bn_relu(x, blk.conv1, blk.bn1, pending)
        z2, par2 = self._conv_bn(a1, blk.conv2, blk.bn2, False, pending)
        r, rpar = x, None
        if blk.downsample is not None:
            r, rpar = self._conv_bn(x, blk.downsample[0], blk.downsample[1], False, pending)
        return bn_add_relu(z2, par2, r, rpar)

    def _encode(self, x_seq: Tensor, pending: list):
        """f32 [B,T,2,H,W] -> (f1 .. f5), 16-bit NHWC with image ``t*B + b``, at H/2 .. H/32."""
        enc = self.encoder
        f1 = self._conv_bn_relu(im2col7x7s2_first(x_seq), enc.conv1, enc.bn1, pending, im2col=True)
        feats, a = [f1], maxpool3s2(f1)
        for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            for blk in layer:
                a = self._block(a, blk, pending)
            feats.append(a)
        return feats

    # -- decoder --------------------------------------------------------------------------------
    @staticmethod
    def _stage(seq: nn.Sequential, x0: Tensor, x1: Optional[Tensor], c_valid, pending: list) -> Tensor:
        conv, bn = seq[0], seq[1]
        training, mom = _bn_mode(bn)
        a = ops.ConvBNReLU.apply(x0, x1, conv.weight, None, bn.weight, bn.bias, bn.running_mean, bn.running_var, tuple(c_valid), (0, 0), 1,
                                 training, mom, bn.eps, False)
        if training and bn.num_batches_tracked is not None:
            pending.append((bn.num_batches_tracked, 1))
        return a

    def forward(self, x_seq: Tensor):
        if not isinstance(x_seq, torch.Tensor) or not x_seq.is_cuda:
            raise UclstmError("PretrainedTemporalUNet: a HIP device tensor is required (this package has no CPU path)")
        if x_seq.dim() != 5 or x_seq.shape[2] != ENCODER_CHANNELS[0]:
            raise UclstmError(f"PretrainedTemporalUNet: expected [B, T, {ENCODER_CHANNELS[0]}, H, W], got {tuple(x_seq.shape)}")
        B, T, _, H, W = x_seq.shape
        if H % 32 or W % 32:
            raise UclstmError(f"PretrainedTemporalUNet: H and W must be multiples of 32 (five stride-2 stages), got {H} x {W}")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.encoder.parameters()):
            raise UclstmError("PretrainedTemporalUNet: training an unfrozen encoder is not supported (no strided input-gradient or "
                              "weight-gradient GEMM): construct with freeze_encoder=True, or run under torch.no_grad()")
        pending: list = []
        try:
            return self._forward(x_seq.contiguous().float(), pending), None
        finally:
            if pending:
                modules._flush_counters(pending)
            ops.join_forward_side(x_seq.device)          # BatchNorm running statistics were updated on the second stream

    def _forward(self, x_seq: Tensor, pending: list) -> Tensor:
        B, T, _, H, W = x_seq.shape
        with torch.no_grad():
            feats = self._encode(x_seq, pending)

        def run(lstm: ConvLSTM, f: Tensor) -> Tensor:          # [T*B,h,w,C] -> the last layer's h for all steps, same shape
            out, _ = lstm.seq_nhwc(f.view(T, B, *f.shape[1:]), None)
            return out.reshape(T * B, *out.shape[2:])

        x = run(self.lstm, feats[4])
        skips = [run(self.lstm_skips[j], feats[j - 1]) for j in (4, 3, 2, 1)] + [None]
        for blk, skip in zip(self.decoder.blocks, skips):
            cin, cskip, cout = blk.channels
            up = Upsample2.apply(x)
            x = self._stage(blk.conv1, up, skip, (cin, cskip) if skip is not None else (cin,), pending)
            x = self._stage(blk.conv2, x, None, (cout,), pending)
        conv = self.head[0]
        y = Head3x3.apply(x, conv.weight, conv.bias)
        return y.view(T, B, self.out_channels, H, W).transpose(0, 1)
