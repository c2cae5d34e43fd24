"""Helpers of the PretrainedTemporalUNet tests that need no GPU (plain torch on the CPU): the state-dict key / shape table of the
reference's ``resnet18_frozen_*`` checkpoints (train/resnet18.py:26-74 over smp.Unet("resnet18", in_channels=2,
decoder_channels=(256,128,64,32,16))), a seeded state generator, a FUNCTIONAL RESTATEMENT of the model's forward pass, the
single-stage gradient helpers (``stage_grads`` / ``report``) with the seeded decoder cases built on them, and f64 references of the
kernels of csrc/resnet.hip with their counted bounds.

The yardstick of the model tests is this restatement, written for the tests from the reference's forward (train/resnet18.py:76-139),
torchvision's BasicBlock and smp's decoder block as the issue states them -- not a fixture produced by the reference: smp is not
available where the fixtures are made, so no golden file exists for the encoder or the decoder.  It is built from F.conv2d /
F.batch_norm / F.max_pool2d / F.interpolate(mode="nearest") and the ConvLSTM equations (train/unet.py:21-36).
"""
import contextlib
import functools

import torch
import torch.nn.functional as F

from conftest import per_tensor_grad_report, rel_l2

ENC = (2, 64, 64, 128, 256, 512)
DEC_IN, DEC_SKIP, DEC_OUT = (512, 256, 128, 64, 32), (256, 128, 64, 64, 0), (256, 128, 64, 32, 16)
U32 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------
# key / shape table
# ---------------------------------------------------------------------------------------------
def _bn(prefix, c):
    return {prefix + "weight": (c,), prefix + "bias": (c,), prefix + "running_mean": (c,), prefix + "running_var": (c,),
            prefix + "num_batches_tracked": ()}


def encoder_table():
    t = {"conv1.weight": (64, 2, 7, 7), **_bn("bn1.", 64)}
    cin = 64
    for li, c in enumerate((64, 128, 256, 512), start=1):
        for b in range(2):
            p = f"layer{li}.{b}."
            t[p + "conv1.weight"] = (c, cin if b == 0 else c, 3, 3)
            t.update(_bn(p + "bn1.", c))
            t[p + "conv2.weight"] = (c, c, 3, 3)
            t.update(_bn(p + "bn2.", c))
            if b == 0 and li > 1:
                t[p + "downsample.0.weight"] = (c, cin, 1, 1)
                t.update(_bn(p + "downsample.1.", c))
        cin = c
    return t


def decoder_table():
    t = {}
    for i, (ci, cs, co) in enumerate(zip(DEC_IN, DEC_SKIP, DEC_OUT)):
        t[f"blocks.{i}.conv1.0.weight"] = (co, ci + cs, 3, 3)
        t.update(_bn(f"blocks.{i}.conv1.1.", co))
        t[f"blocks.{i}.conv2.0.weight"] = (co, co, 3, 3)
        t.update(_bn(f"blocks.{i}.conv2.1.", co))
    return t


def lstm_table(prefix, ch, layers):
    t = {}
    for l in range(layers):
        t[f"{prefix}layers.{l}.conv.weight"] = (4 * ch, 2 * ch, 3, 3)
        t[f"{prefix}layers.{l}.conv.bias"] = (4 * ch,)
    return t


def key_table(out_channels=1, lstm_layers=1):
    """name -> shape of every state_dict entry, both prefixes of the shared parts included."""
    t = {}
    head = {"0.weight": (out_channels, 16, 3, 3), "0.bias": (out_channels,)}
    for pa, pb, part in (("base_model.encoder.", "encoder.", encoder_table()), ("base_model.decoder.", "decoder.", decoder_table()),
                         ("base_model.segmentation_head.", "head.", head)):
        for k, s in part.items():
            t[pa + k] = s
            t[pb + k] = s
    t.update(lstm_table("lstm.", 512, lstm_layers))
    for j, ch in enumerate(ENC[:-1]):
        t.update(lstm_table(f"lstm_skips.{j}.", ch, lstm_layers))
    return t


ALIASES = (("base_model.encoder.", "encoder."), ("base_model.decoder.", "decoder."), ("base_model.segmentation_head.", "head."))


def is_buffer(k):
    return k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def is_trainable(k, freeze_encoder=True):
    """Keys (short prefixes only) of the tensors a default model trains."""
    if is_buffer(k) or k.startswith("base_model.") or k.startswith("lstm_skips.0."):
        return False
    return not (freeze_encoder and k.startswith("encoder."))


def make_state(seed, out_channels=1, lstm_layers=1):
    """A full state_dict (f32, CPU): fan-in scaled weights, gamma in [0.5, 1.5], non-trivial running statistics."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in key_table(out_channels, lstm_layers).items():
        if k.startswith("base_model."):
            continue
        if k.endswith("num_batches_tracked"):
            v = torch.tensor(3, dtype=torch.int64)
        elif k.endswith("running_mean"):
            v = torch.randn(shape, generator=g) * 0.2
        elif k.endswith("running_var"):
            v = torch.rand(shape, generator=g) * 1.0 + 0.5
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            v = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
            if ".conv.weight" in k:          # ConvLSTM gates: keep the pre-activations O(1)
                v = v * 0.7
        elif k.endswith(".weight"):          # BatchNorm gamma
            v = torch.rand(shape, generator=g) + 0.5
        else:                                # BatchNorm beta, conv / gate biases
            v = torch.randn(shape, generator=g) * 0.1
        sd[k] = v
    for pa, pb in ALIASES:
        for k in [k for k in sd if k.startswith(pb)]:
            sd[pa + k[len(pb):]] = sd[k]
    return sd


def torchvision_resnet18_state(seed):
    """A torchvision-layout ResNet18 state_dict (3-channel conv1, fc.*), random: what ``encoder_weights`` accepts."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in encoder_table().items():
        if k == "conv1.weight":
            shape = (64, 3, 7, 7)
        sd[k] = torch.tensor(0, dtype=torch.int64) if k.endswith("num_batches_tracked") else \
            (torch.rand(shape, generator=g) + 0.5 if k.endswith("running_var") else torch.randn(shape, generator=g) * 0.1)
    sd["fc.weight"], sd["fc.bias"] = torch.randn(1000, 512, generator=g), torch.randn(1000, generator=g)
    return sd


# ---------------------------------------------------------------------------------------------
# functional restatement of the model
# ---------------------------------------------------------------------------------------------
class _Ref:
    def __init__(self, sd, training, dtype):
        self.p = {k: (v if (v.dtype == dtype or not v.is_floating_point()) else v.to(dtype)) for k, v in sd.items() if not k.startswith("base_model.")}
        self.training, self.dtype, self.buffers = training, dtype, {}

    def bn(self, x, prefix):
        p = self.p
        rm, rv = p[prefix + "running_mean"].detach().clone(), p[prefix + "running_var"].detach().clone()
        y = F.batch_norm(x, rm, rv, p[prefix + "weight"], p[prefix + "bias"], self.training, 0.1, 1e-5)
        if self.training:
            self.buffers[prefix + "running_mean"], self.buffers[prefix + "running_var"] = rm, rv
            self.buffers[prefix + "num_batches_tracked"] = p[prefix + "num_batches_tracked"] + 1
        return y

    def block(self, x, prefix, stride):
        p = self.p
        out = F.relu(self.bn(F.conv2d(x, p[prefix + "conv1.weight"], None, stride, 1), prefix + "bn1."))
        out = self.bn(F.conv2d(out, p[prefix + "conv2.weight"], None, 1, 1), prefix + "bn2.")
        idt = x
        if prefix + "downsample.0.weight" in p:
            idt = self.bn(F.conv2d(x, p[prefix + "downsample.0.weight"], None, stride, 0), prefix + "downsample.1.")
        return F.relu(out + idt)

    def encoder(self, x):
        p = self.p
        f = [F.relu(self.bn(F.conv2d(x, p["encoder.conv1.weight"], None, 2, 3), "encoder.bn1."))]
        a = F.max_pool2d(f[0], 3, 2, 1)
        for li in range(1, 5):
            for b in range(2):
                a = self.block(a, f"encoder.layer{li}.{b}.", 2 if (b == 0 and li > 1) else 1)
            f.append(a)
        return f

    def convlstm(self, seq, prefix):
        """seq [B,T,C,h,w] -> the last layer's h, same shape (train/unet.py:46-60, zero initial state)."""
        p, out, l = self.p, seq, 0
        while f"{prefix}layers.{l}.conv.weight" in p:
            w, b = p[f"{prefix}layers.{l}.conv.weight"], p[f"{prefix}layers.{l}.conv.bias"]
            hd = w.shape[0] // 4
            h = out.new_zeros(out.shape[0], hd, *out.shape[3:])
            c, hs = h, []
            for t in range(out.shape[1]):
                i, f, g, o = torch.chunk(F.conv2d(torch.cat([out[:, t], h], 1), w, b, 1, 1), 4, 1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                hs.append(h)
            out, l = torch.stack(hs, 1), l + 1
        return out

    def forward(self, x):
        B, T = x.shape[:2]
        feats = self.encoder(x.reshape(B * T, *x.shape[2:]).to(self.dtype))

        def temporal(f, prefix):
            return self.convlstm(f.view(B, T, *f.shape[1:]), prefix).reshape(B * T, *f.shape[1:])

        a = temporal(feats[4], "lstm.")
        y = self.decoder(a, [temporal(feats[j - 1], f"lstm_skips.{j}.") for j in (4, 3, 2, 1)] + [None])
        return y.view(B, T, *y.shape[1:])

    def concat(self, up, skip):
        return torch.cat([up, skip], 1)

    def decoder_block(self, x, skip, i):
        """smp's DecoderBlock ``i``: nearest x2, cat([x, skip]) (``skip`` None: the last block), conv3x3 / BatchNorm / ReLU twice."""
        a = F.interpolate(x, scale_factor=2, mode="nearest")
        if skip is not None:
            a = self.concat(a, skip)
        for c in ("conv1", "conv2"):
            a = F.relu(self.bn(F.conv2d(a, self.p[f"decoder.blocks.{i}.{c}.0.weight"], None, 1, 1), f"decoder.blocks.{i}.{c}.1."))
        return a

    def decoder(self, x, skips):
        """The five blocks on the bottleneck ``x`` and ``skips`` (deepest first, None for the last block), then the head."""
        for i, skip in enumerate(skips):
            x = self.decoder_block(x, skip, i)
        return F.conv2d(x, self.p["head.0.weight"], self.p["head.0.bias"], 1, 1)


def forward_ref(sd, x, training, dtype=torch.float64, autocast=None):
    """(y [B,T,out,H,W], updated BatchNorm buffers by short key).  ``autocast``: run under torch.autocast("cpu", dtype=autocast)
    (then ``dtype`` should be float32): the anchor of the model tests' tolerances."""
    ref = _Ref(sd, training, dtype)
    ctx = torch.autocast("cpu", dtype=autocast) if autocast is not None else contextlib.nullcontext()
    with ctx:
        y = ref.forward(x)
    return y, ref.buffers


def loss_ref(y_pred, y, mask):
    """main.py:28-72 with the mask (the oracle's restatement, repeated here so that the helper stands alone)."""
    ad = (y_pred - y).abs()
    w = 1.0 + 4.0 * y.abs() ** 3
    l1 = (ad * mask * w).sum() / ((mask * w).sum() + 1e-8)
    H, W = y.shape[-2], y.shape[-1]
    gd = ((y_pred[..., :, 1:] - y_pred[..., :, :-1]) - (y[..., :, 1:] - y[..., :, :-1]))[..., :H - 1, :W - 1].abs() + \
         ((y_pred[..., 1:, :] - y_pred[..., :-1, :]) - (y[..., 1:, :] - y[..., :-1, :]))[..., :H - 1, :W - 1].abs()
    mc = mask[..., :H - 1, :W - 1]
    return l1 + 0.005 * (gd * mc).sum() / (mc.sum() + 1e-8)


def train_ref(sd, x, y, mask, dtype=torch.float64, autocast=None):
    """Train-mode forward + loss + gradients of every trainable tensor: (y_pred, loss, {key: grad}, buffers)."""
    names = [k for k in sd if is_trainable(k)]
    leaves = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in names}
    yp, buffers = forward_ref({**sd, **leaves}, x, True, dtype, autocast)
    loss = loss_ref(yp.to(dtype), y.to(dtype), mask.to(dtype))
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return yp.detach(), loss.detach(), dict(zip(names, grads)), buffers


def make_batch(seed, B, T, H, W, out_channels=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 2, H, W, generator=g)
    y = torch.randn(B, T, out_channels, H, W, generator=g) * 0.5
    mask = (torch.rand(B, T, out_channels, H, W, generator=g) > 0.2).float()
    return x, y, mask


# ---------------------------------------------------------------------------------------------
# single stages against f64: gradients of sum(out * gout), and the restatement's own reduced-precision drift as the anchor
# ---------------------------------------------------------------------------------------------
def stage_grads(sd, prefix, x, gouts, run, dtype, autocast, training=True, ref_cls=None, keep=None):
    """Gradients of sum(out_i * gout_i) with respect to x and every parameter under ``prefix`` (one prefix or a tuple of them);
    ``run(ref, x)`` -> outputs.  ``x``: one tensor, whose gradient is returned as "x", or a dict name -> tensor (None entries stay
    None and get no gradient): ``run`` then gets the dict of leaves.  ``training``: the BatchNorm mode of the restatement;
    ``ref_cls``: a subclass of _Ref to run instead; ``keep`` (a dict) receives "outs" and "buffers"."""
    names = [k for k in sd if k.startswith(prefix) and not is_buffer(k)]
    leaves = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in names}
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    xs = {k: leaf(v) for k, v in x.items()} if isinstance(x, dict) else {"x": leaf(x)}
    ref = (ref_cls or _Ref)({**sd, **leaves}, training, dtype)
    with (torch.autocast("cpu", dtype=autocast) if autocast is not None else contextlib.nullcontext()):
        outs = run(ref, xs if isinstance(x, dict) else xs["x"])
    loss = sum((o.to(dtype) * g.to(dtype)).sum() for o, g in zip(outs, gouts))
    wrt = {**{k: v for k, v in xs.items() if v is not None}, **leaves}
    grads = torch.autograd.grad(loss, list(wrt.values()), allow_unused=True)
    if keep is not None:
        keep.update(outs=[o.detach() for o in outs], buffers=dict(ref.buffers))
    return dict(zip(wrt, grads))


def report(what, got, want, anchor, label=lambda k: k.split(".", 3)[-1]):
    """conftest.per_tensor_grad_report with its defaults over the tensors of ``want``: prints the ratios (``label``: how a key is
    printed; by default without its stage prefix), raises on a failure."""
    names = list(want)
    bad, rows, med = per_tensor_grad_report(names, got, want, [float(want[k].norm()) for k in names], [anchor[k] for k in names])
    print(f"[parity] {what}: median rel-L2 / anchor {med:.3f} (bound 1.25); (rel-L2 / bound): " +
          "; ".join(f"{label(k)} {rel:.4f}/{bound:.4f}" for _, k, rel, bound, _, z in rows if not z))
    assert not bad, " | ".join(bad[:8])


# ---------------------------------------------------------------------------------------------
# the decoder, one block at a time and as a chain: seeded inputs, the f64 reference and the autocast anchor of every case of
# tests/test_gpu_resnet_decoder.py, computed on the CPU (tests/test_resnet_host.py checks the anchors without a GPU)
# ---------------------------------------------------------------------------------------------
DEC_STATE_SEED = 101
DEC_DTYPES = (torch.bfloat16, torch.float16)
DEC_MODES = ("train", "eval")                      # BatchNorm with batch statistics / with running statistics, both with a backward pass
DEC_ANCHOR_CAP, DEC_CHAIN_ANCHOR_CAP = 0.12, 0.30   # conditions on the INPUTS: with them the per-tensor bound 2.5 x anchor stays <= 0.30 / 0.75
DEC_CHAIN_N = 4
# forward floor of one stage in bf16 (tests/test_gpu_ops.py::test_conv_bn_relu_train_fwd_bwd_two_groups); fp16 has three more mantissa bits
DEC_OUT_FLOOR = {torch.bfloat16: 6e-3, torch.float16: 6e-3 / 8}


def decoder_block_shapes(i):
    """(n, h, w) of the input of block ``i`` (its skip and its output are 2h x 2w): the block's own shape in the model's smallest
    test case (B2 T2, 64 x 64), and 3 x (3, 5) -> 180 output pixels: a partial tile in every direction, non-square, an odd image count."""
    return [(4, 2 ** (i + 1), 2 ** (i + 1)), (3, 3, 5)]


@functools.lru_cache(maxsize=None)
def decoder_state():
    """The decoder's and the head's entries of make_state(DEC_STATE_SEED): shared, never modified."""
    return {k: v for k, v in make_state(DEC_STATE_SEED, 1, 1).items() if k.startswith(("decoder.", "head."))}


def decoder_block_inputs(i, shape, dtype):
    """(x [n,cin,h,w], skip [n,cskip,2h,2w] or None, gout [n,cout,2h,2w]): f32 values that ``dtype`` holds exactly, so that the
    device and the reference start from the same numbers (gout too: autograd hands it to the stage in the activation's dtype)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(4000 + 100 * i + 10 * n + h)
    q = lambda t: t.to(dtype).float()
    x = q(torch.randn(n, DEC_IN[i], h, w, generator=g))
    skip = q(torch.randn(n, DEC_SKIP[i], 2 * h, 2 * w, generator=g)) if DEC_SKIP[i] else None
    return x, skip, q(torch.randn(n, DEC_OUT[i], 2 * h, 2 * w, generator=g))


def _anchored(sd, prefix, inputs, gouts, run, dtype, mode, ref_cls=None):
    """The f64 result of one case and the drift of the same restatement in f32 under torch.autocast("cpu", dtype) against it."""
    training, k64, k16 = mode == "train", {}, {}
    grads = stage_grads(sd, prefix, inputs, gouts, run, torch.float64, None, training, ref_cls, k64)
    drift = stage_grads(sd, prefix, inputs, gouts, run, torch.float32, dtype, training, ref_cls, k16)
    fbuf = [k for k in k64["buffers"] if not k.endswith("num_batches_tracked")]
    return dict(sd=sd, inputs=inputs, gouts=gouts, out=k64["outs"][0], grads=grads, buffers=k64["buffers"],
                anchor_out=rel_l2(k16["outs"][0], k64["outs"][0]), anchor_grads={k: rel_l2(drift[k], grads[k]) for k in grads},
                anchor_buffers={k: rel_l2(k16["buffers"][k], k64["buffers"][k]) for k in fbuf})


def decoder_block_reference(i, shape, dtype, mode, ref_cls=None):
    """Block ``i`` alone: gradients of sum(out * gout) for x, skip and the block's six parameters, the output, the updated buffers."""
    x, skip, gout = decoder_block_inputs(i, shape, dtype)
    run = lambda ref, xs: [ref.decoder_block(xs["x"], xs["skip"], i)]
    return _anchored(decoder_state(), f"decoder.blocks.{i}.", {"x": x, "skip": skip}, [gout], run, dtype, mode, ref_cls)


def decoder_chain_inputs(dtype):
    """The model's own smallest decoder shapes: a bottleneck of 512 x 2 x 2, four skips, an f32 output gradient [n, 1, 64, 64]."""
    n, g = DEC_CHAIN_N, torch.Generator().manual_seed(4900)
    q = lambda t: t.to(dtype).float()
    inputs = {"x": q(torch.randn(n, DEC_IN[0], 2, 2, generator=g))}
    for i in range(4):
        inputs[f"skip{i}"] = q(torch.randn(n, DEC_SKIP[i], 4 << i, 4 << i, generator=g))
    return inputs, torch.randn(n, 1, 64, 64, generator=g)


def decoder_chain_reference(dtype, mode):
    """The five blocks and the head: gradients for x, the four skips, every decoder.* parameter and head.0.*."""
    inputs, gout = decoder_chain_inputs(dtype)
    run = lambda ref, xs: [ref.decoder(xs["x"], [xs[f"skip{i}"] for i in range(4)] + [None])]
    return _anchored(decoder_state(), ("decoder.", "head."), inputs, [gout], run, dtype, mode)


# shared by the tests of one process: computed once per case, never modified
decoder_block_case = functools.lru_cache(maxsize=None)(decoder_block_reference)
decoder_chain_case = functools.lru_cache(maxsize=None)(decoder_chain_reference)


# ---------------------------------------------------------------------------------------------
# f64 references of the kernels of csrc/resnet.hip (inputs: the 16-bit values the device holds, NHWC) and their bounds
# ---------------------------------------------------------------------------------------------
def u16(dtype):
    """Half a unit in the last place, relative: one rounding to the 16-bit storage type."""
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def round16_bound(ref, mag, dtype, n_f32):
    """|err| of a value computed in f32 with `n_f32` roundings on terms of total magnitude `mag`, then rounded once to 16 bits:
    u16 * |ref| (1 + 2^-10 for the shift of the rounding point by the f32 error), the fp16 subnormal floor 2^-25, n_f32 * 2^-24 * mag."""
    floor = 2.0 ** -25 if dtype == torch.float16 else 0.0
    return (u16(dtype) * (1 + 2.0 ** -10) * ref.abs()).clamp(min=floor) + n_f32 * U32 * mag * (1 + 2 * u16(dtype))


def im2col7_ref(x, B, T, Kp):
    """x f32 [B,T,C,H,W] -> [T*B, Ho, Wo, Kp] (image t*B + b), K = (dy*7 + dx)*C + c."""
    _, _, Cc, H, W = x.shape
    xi = x.transpose(0, 1).reshape(T * B, Cc, H, W)
    cols = F.unfold(xi, 7, padding=3, stride=2)                        # [n, C*49, Ho*Wo], row = c*49 + tap
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cols = cols.view(T * B, Cc, 49, Ho, Wo).permute(0, 3, 4, 2, 1).reshape(T * B, Ho, Wo, 49 * Cc)
    return F.pad(cols, (0, Kp - 49 * Cc))


def nchw(a):
    return a.permute(0, 3, 1, 2)


def nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous()


def maxpool3s2_ref(a):
    return nhwc(F.max_pool2d(nchw(a.double()), 3, 2, 1))


def upsample2_ref(a):
    return nhwc(F.interpolate(nchw(a.double()), scale_factor=2, mode="nearest"))


def upsample2_bwd_ref(d):
    """(sum of the four children, sum of their magnitudes): three f32 additions on the way."""
    d = d.double()
    parts = [d[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    return sum(parts), sum(p.abs() for p in parts)


def bn_add_relu_ref(z, scale, shift, r, rscale, rshift):
    """(value, magnitude of the summed terms).  f32 roundings: product and sum of each affine (2 + 2), the add (1): <= 5."""
    z, r = z.double(), r.double()
    tz = [z * scale.double(), shift.double().expand_as(z)] if scale is not None else [z]
    tr = [r * rscale.double(), rshift.double().expand_as(r)] if rscale is not None else [r]
    terms = tz + tr
    return sum(terms).clamp(min=0.0), sum(t.abs() for t in terms)


def head_fwd_ref(a, w, b, C):
    """a [n,H,W,Cp] 16-bit values, w f32 [Co,C,3,3], b [Co] -> (y [n,Co,H,W], sum |terms|)."""
    x = nchw(a.double())[:, :C]
    y = F.conv2d(x, w.double(), b.double(), 1, 1)
    mag = F.conv2d(x.abs(), w.double().abs(), b.double().abs(), 1, 1)
    return y, mag


def head_bwd_ref(a, w, dy, C, Cp):
    """(da NHWC [n,H,W,Cp] with zero padding channels, its magnitude, dw, its magnitude, db, its magnitude), all f64."""
    x, wd, g = nchw(a.double())[:, :C], w.double(), dy.double()
    da = F.conv_transpose2d(g, wd, None, 1, 1)
    da_mag = F.conv_transpose2d(g.abs(), wd.abs(), None, 1, 1)
    n, Co, H, W = g.shape
    xp = F.pad(x, (1, 1, 1, 1))
    dw, dw_mag = torch.zeros_like(wd), torch.zeros_like(wd)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + H, kx:kx + W]
            dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, win)
            dw_mag[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g.abs(), win.abs())
    pad = (0, Cp - C)
    return F.pad(nhwc(da), pad), F.pad(nhwc(da_mag), pad), dw, dw_mag, g.sum((0, 2, 3)), g.abs().sum((0, 2, 3))
