"""Helpers of tests/test_gpu_grad_routes.py that need no GPU: the case table, the f64 references of every parameter gradient and
the checker of "what lies in param.grad afterwards".

A parameter gradient reaches ``param.grad`` by one of two routes (ops.py): the operator returns it and autograd accumulates it,
or a backward kernel adds straight into an attached contiguous f32 buffer (direct_grad, direct_grad_pair, bias_grad_from_colsum,
wgrad_into_param, uclstm_bn_bwd_param_grads, the fused head, Head3x3).  Either way PyTorch's contract is +=: after a backward pass
the buffer holds what it held before plus the gradient.  Every reference here therefore yields, per parameter,

    G64   the gradient in f64 from the 16-bit-rounded inputs the kernel multiplies, and
    T64   the sum of the magnitudes of the terms of each element of G64 (the yardstick of every sum bound in this repository),

and ``check_param`` holds the buffer to  |grad - (P + sum_k G64_k)| <= sum_k b_k (T64_k + |P + sum_{j<k} G64_j|)  where P is the
attached start value (0 when nothing was attached), k runs over the backward passes / uses that added into the buffer and b_k is
the bound the kernel behind that gradient already holds at the C ABI (imported by the GPU test, not restated).  P is drawn once
per case from N(0, 1) and scaled to rms(G64): a dropped or doubled P is an O(1) error while ulp(P) stays far below b * T64.

References that are already written elsewhere are imported: boundary_cases (1x1 output convolution, spatial attention),
resnet_cases (the 3x3 head), recurrence_cases / wgrad_cases (ConvLSTM weight gradient through the pack descriptors).  Where a
gradient is a function of tensors only the device has (the BatchNorm stage's dz and backward sums, the recurrence's dgates) the
reference takes those stored tensors as inputs, as tests/recurrence_cases.py does; the full f64 chains of this file
(``stage_chain``, ``lstm_chain``) give the scale of P and the host tests their mutants.
tests/test_grad_route_cases_host.py pins every restatement to PyTorch's own f64 modules.
"""
from dataclasses import dataclass
from typing import Sequence

import torch
import torch.nn.functional as F

import boundary_cases as BC
import resnet_cases as RC

F64 = torch.float64
MARK = 0.25          # fill of a frozen parameter's attached buffer (tests/test_gpu_conv_stage.py uses the same value)


def r16(t, dtype):
    return t.to(dtype).float()


def nchw(a, C):
    """NHWC with padded channels -> f64 NCHW of the C valid ones."""
    return a.double()[..., :C].permute(0, 3, 1, 2).contiguous()


def pad_last(t, Cp):
    out = torch.zeros(t.shape[:-1] + (Cp,), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def cpad(c):
    return (c + 7) // 8 * 8


def _wgrad_of(conv, x, g, wshape):
    """Gradient of sum(conv(x, w) * g) with respect to w for an operator linear in w (so w's value does not matter)."""
    w = torch.zeros(wshape, dtype=F64, requires_grad=True)
    return torch.autograd.grad(conv(x, w), w, g)[0]


def _with_terms(conv, x, g, wshape):
    return _wgrad_of(conv, x, g, wshape), _wgrad_of(conv, x.abs(), g.abs(), wshape)


# ---------------------------------------------------------------------------------------------
# references: {parameter name: (G64, T64)}
# ---------------------------------------------------------------------------------------------
def convt_ref(x, wshape, du, has_bias=True):
    """ConvTranspose2d(k 2, stride 2): x [N,h,w,Cip], du [N,2h,2w,Cop] (16-bit values), weight [Ci,Co,2,2]."""
    Ci, Co = wshape[0], wshape[1]
    xs, g = nchw(x, Ci), nchw(du, Co)
    out = {"weight": _with_terms(lambda a, w: F.conv_transpose2d(a, w, None, stride=2), xs, g, wshape)}
    if has_bias:
        out["bias"] = (g.sum((0, 2, 3)), g.abs().sum((0, 2, 3)))
    return out


def outconv_ref(a, w, dy, has_bias=True):
    """1x1 output convolution: a [N,H,W,Cp] 16-bit values, w [Co,Ci,1,1], dy f32 [N,Co,H,W] (boundary_cases.outconv_bwd_ref)."""
    N, H, W, Cp = a.shape
    Co, Ci = w.shape[0], w.shape[1]
    _, _, dw, tw, db, tb = BC.outconv_bwd_ref(a.reshape(N * H * W, Cp), w.reshape(Co, Ci), dy.reshape(N, Co, H * W), Cp)
    out = {"weight": (dw.view(Co, Ci, 1, 1), tw.view(Co, Ci, 1, 1))}
    if has_bias:
        out["bias"] = (db, tb)
    return out


def attn_ref(x, w, C, dout):
    """Spatial attention: x, dout [N,H,W,Cp] 16-bit values, w [1,2,k,k] (boundary_cases.attn_*).  T64 expands every inner sum:
    sum_p (sum_c |x dout|) att (1 - att) * (sum_c |x| / C, |max|)."""
    k = w.shape[-1]
    fwd = BC.attn_fwd_ref(x, w[0], C)
    bwd = BC.attn_bwd_ref(x, dout, w[0], C, fwd)
    att = fwd["att"]
    dpre_mag = (x.double() * dout.double()).abs().sum(-1) * att * (1.0 - att)
    _, _, _, mean_mag = BC.attn_desc_ref(x, C)
    terms, _ = BC.attn_dw_ref(dpre_mag, torch.stack((mean_mag, fwd["max"].abs()), -1), k)
    return {"weight": (bwd["dw"][None], terms[None])}


def head3x3_ref(a, w, dy, has_bias=True):
    """The 3x3 head: a [N,H,W,Cp] 16-bit values, w [Co,C,3,3], dy f32 [N,Co,H,W] (resnet_cases.head_bwd_ref)."""
    C = w.shape[1]
    _, _, dw, tw, db, tb = RC.head_bwd_ref(a, w, dy, C, a.shape[-1])
    out = {"weight": (dw, tw)}
    if has_bias:
        out["bias"] = (db, tb)
    return out


def concat_sources(srcs, H, W):
    """srcs [(x NHWC, valid channels, offY, offX)] -> f64 NCHW [N, sum C, H, W], every source placed inside the H x W frame."""
    parts = []
    for x, c, oy, ox in srcs:
        v = nchw(x, c)
        full = torch.zeros(v.shape[0], c, H, W, dtype=F64)
        full[:, :, oy:oy + v.shape[2], ox:ox + v.shape[3]] = v
        parts.append(full)
    return torch.cat(parts, 1)


def conv3x3_wgrad_ref(srcs, dz, Co):
    """Weight gradient of conv3x3 pad 1 over the channel concat of ``srcs`` from dz [N,H,W,Cop] (16-bit values)."""
    N, H, W, _ = dz.shape
    x = concat_sources(srcs, H, W)
    return _with_terms(lambda a, w: F.conv2d(a, w, None, padding=1), x, nchw(dz, Co), (Co, x.shape[1], 3, 3))


def bn_param_ref(sums, Co):
    """uclstm_bn_bwd_param_grads: dbeta = sum_g sums[g][c][0], dgamma = sum_g sums[g][c][1] (sums f32 [groups, Cop, 2])."""
    s = sums.double()[:, :Co]
    return {"beta": (s[..., 0].sum(0), s[..., 0].abs().sum(0)), "gamma": (s[..., 1].sum(0), s[..., 1].abs().sum(0))}


def colsum_ref(a, valid):
    a2 = a.double().reshape(-1, a.shape[-1])[:, :valid]
    return a2.sum(0), a2.abs().sum(0)


def fused_head_ref(a, dy, Co):
    """The 1x1 head fused behind a BatchNorm stage: a [N,H,W,Cop] = the stage's 16-bit activation, dy f32 [N,1,H,W]."""
    a2 = a.double().reshape(-1, a.shape[-1])[:, :Co]
    g = dy.double().reshape(-1, 1)
    return {"head_w": ((g * a2).sum(0).view(1, Co, 1, 1), (g * a2).abs().sum(0).view(1, Co, 1, 1)),
            "head_b": (g.sum().view(1), g.abs().sum().view(1))}


# ---------------------------------------------------------------------------------------------
# full f64 chains (the scale of P, the host tests)
# ---------------------------------------------------------------------------------------------
def stage_chain(x, weight, bias, gamma, beta, groups, training, da, eps=1e-5, rm=None, rv=None, head=None, dy=None):
    """conv3x3 + bias -> BatchNorm over ``groups`` image groups (or the running statistics) -> ReLU [-> 1x1 head] written out with
    the header's backward formulas: x f64 NCHW, da f64 NCHW (or dy [N,1,H,W] with ``head`` = (head_w, head_b)).
    -> dict(z, a, dz NCHW, sums [groups, Co, 2], grads {name: G64})."""
    x, w = x.double(), weight.double()
    N, Co = x.shape[0], w.shape[0]
    z = F.conv2d(x, w, None if bias is None else bias.double(), padding=1)
    G = groups if training else 1
    zg = z.view(G, N // G, Co, *z.shape[2:])
    n = zg.shape[1] * zg.shape[3] * zg.shape[4]
    if training:
        mean = zg.mean((1, 3, 4), keepdim=True)
        var = ((zg - mean) ** 2).mean((1, 3, 4), keepdim=True)
    else:
        mean, var = rm.double().view(1, 1, Co, 1, 1), rv.double().view(1, 1, Co, 1, 1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (zg - mean) * rstd
    ga, be = gamma.double().view(1, 1, Co, 1, 1), beta.double().view(1, 1, Co, 1, 1)
    y = xhat * ga + be
    a = y.clamp(min=0.0)
    grads = {}
    if head is not None:
        hw, g = head[0].double().view(1, 1, Co, 1, 1), dy.double().view(G, N // G, 1, *z.shape[2:])
        da_g = g * hw
        grads["head_w"] = (g * a).sum((0, 1, 3, 4)).view(1, Co, 1, 1)
        grads["head_b"] = g.sum().view(1)
    else:
        da_g = da.double().view_as(zg)
    g0 = torch.where(y > 0, da_g, torch.zeros_like(da_g))
    s1, s2 = g0.sum((1, 3, 4), keepdim=True), (g0 * xhat).sum((1, 3, 4), keepdim=True)
    dz = ga * rstd * ((g0 - s1 / n - xhat * s2 / n) if training else g0)
    dz = dz.reshape(z.shape)
    sums = torch.stack((s1.reshape(G, Co), s2.reshape(G, Co)), -1)
    grads["weight"] = _wgrad_of(lambda t, ww: F.conv2d(t, ww, None, padding=1), x, dz, w.shape)
    grads["beta"], grads["gamma"] = sums[..., 0].sum(0), sums[..., 1].sum(0)
    if bias is not None:
        grads["bias"] = dz.sum((0, 2, 3))
    return dict(z=z, a=a.reshape(z.shape), dz=dz, sums=sums, grads=grads)


def lstm_chain(xs, weight, bias, Hd, dhs, per_use=False):
    """The ConvLSTM cell of the reference applied to xs[0..T-1] (f64 NCHW) from the zero state, loss = sum_t <h_t, dhs[t]>: the
    gate order of the convolution's output channels is (i, f, g, o).  -> {weight, bias: G64}; ``per_use``: a list with the
    contribution of every timestep (the use of the shared module at that step) instead of their sum."""
    T = len(xs)
    ws = [weight.double().clone().requires_grad_(True) for _ in range(T)]
    bs = [bias.double().clone().requires_grad_(True) for _ in range(T)]
    B, _, H, W = xs[0].shape
    h = torch.zeros(B, Hd, H, W, dtype=F64)
    c = torch.zeros_like(h)
    loss = 0.0
    for t in range(T):
        pre = F.conv2d(torch.cat((xs[t].double(), h), 1), ws[t], bs[t], padding=weight.shape[-1] // 2)
        i, f, g, o = pre.split(Hd, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        loss = loss + (h * dhs[t].double()).sum()
    gs = torch.autograd.grad(loss, ws + bs)
    uses = [{"weight": gs[t], "bias": gs[T + t]} for t in range(T)]
    if per_use:
        return uses
    return {"weight": sum(u["weight"] for u in uses), "bias": sum(u["bias"] for u in uses)}


# ---------------------------------------------------------------------------------------------
# start values and the checker
# ---------------------------------------------------------------------------------------------
def draw_P(G, seed):
    """{name: P}: N(0, 1) scaled to rms(G64) of that parameter (to 1 where the gradient is analytically zero: the bias in front of
    training-mode BatchNorm), as f32."""
    gen = torch.Generator().manual_seed(9100 + seed)
    out = {}
    for k in sorted(G):
        g = G[k][0] if isinstance(G[k], tuple) else G[k]
        rms = float(g.double().pow(2).mean().sqrt())
        out[k] = (torch.randn(g.shape, generator=gen) * (rms if rms > 1e-9 else 1.0)).float()          # (f64 cancellation noise is ~1e-16)
    return out


@dataclass
class Add:
    """One addition into a gradient buffer: the f64 gradient, the sum of the magnitudes of its terms, the kernel's bound."""
    G: torch.Tensor
    T: torch.Tensor
    b: float


def expected(P, adds: Sequence[Add]):
    """(P + sum G, sum_k b_k (T_k + |what the buffer held before addition k|) + 1e-30), f64, flat."""
    base = torch.zeros_like(adds[0].G.double().reshape(-1)) if P is None else P.double().reshape(-1).clone()
    bound = torch.zeros_like(base)
    for a in adds:
        bound = bound + a.b * (a.T.double().reshape(-1) + base.abs())
        base = base + a.G.double().reshape(-1)
    return base, bound + 1e-30


class RouteError(AssertionError):
    pass


def check_param(what, name, route, got, P, adds: Sequence[Add]):
    """``got``: param.grad after the run (None: no gradient at all).  Returns the worst |err| / bound; raises RouteError naming the
    parameter and the route otherwise."""
    tag = f"{what}: {name} [{route} route]"
    if got is None:
        raise RouteError(f"{tag}: no gradient arrived (.grad is None)")
    want, bound = expected(P, adds)
    g = got.detach().double().cpu().reshape(-1)
    if g.shape != want.shape:
        raise RouteError(f"{tag}: gradient of {tuple(got.shape)} for {want.numel()} elements")
    if not bool(torch.isfinite(g).all()):
        raise RouteError(f"{tag}: non-finite gradient")
    ratio = float(((g - want).abs() / bound).max())
    if ratio > 1.0:
        p = torch.zeros_like(want) if P is None else P.double().reshape(-1)
        tot = want - p
        hints = {"stored instead of added (P lost)": tot, "P added twice": want + p}
        for k in range(len(adds)):
            hints[f"addition {k} of {len(adds)} missing"] = want - adds[k].G.double().reshape(-1)
        hint = ""
        for h, v in hints.items():
            if float(((g - v).abs() / bound).max()) <= 1.0:
                hint = f" -- it equals the result with {h}"
        raise RouteError(f"{tag}: |grad - (P + G64)| is {ratio:.3g} x its bound, worst |err| {float((g - want).abs().max()):.3e}{hint}")
    return ratio


def check_frozen(what, name, route, got, attached):
    """A frozen parameter: an attached buffer keeps the MARK fill bit for bit, without one .grad stays None."""
    tag = f"{what}: frozen {name} [{route} route]"
    if not attached:
        if got is not None:
            raise RouteError(f"{tag}: got a gradient although it is frozen and nothing was attached")
        return
    if got is None or not torch.equal(got.detach().cpu(), torch.full(got.shape, MARK, dtype=got.dtype)):
        raise RouteError(f"{tag}: its attached buffer was written")


# ---------------------------------------------------------------------------------------------
# case table: the smallest shapes at which each route decision can go wrong
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConvTCase:
    Ci: int
    Co: int
    N: int = 2
    h: int = 3
    w: int = 5

    @property
    def name(self):
        return f"convt{self.Ci}-{self.Co}"

    @property
    def bias_direct(self):          # bias_grad_from_colsum: the buffer must have exactly Cp elements
        return self.Co % 8 == 0


CONVT_CASES = [ConvTCase(16, 8), ConvTCase(16, 12)]


@dataclass(frozen=True)
class OutConvCase:
    Ci: int
    Co: int
    N: int = 2
    H: int = 5
    W: int = 7

    @property
    def name(self):
        return f"outconv{self.Ci}-{self.Co}"


OUTCONV_CASES = [OutConvCase(ci, co) for ci in (8, 12) for co in (1, 3)]
ATTACH_SETS = [("weight", "bias"), ("weight",), ("bias",)]          # direct_grad_pair is all-or-nothing


@dataclass(frozen=True)
class AttnCase:
    k: int
    N: int = 2
    H: int = 6
    W: int = 5
    C: int = 16

    @property
    def name(self):
        return f"attn-k{self.k}"


ATTN_CASES = [AttnCase(3), AttnCase(7)]


@dataclass(frozen=True)
class StageCase:
    """ConvBNReLU: N images in ``groups`` BatchNorm groups; variant plain | pool | head | im2col | two (sources, the second one
    6 x 6 centred at (1, 1)).  im2col is the first layer: its input has 2 channels (9 * Ci <= 64)."""
    variant: str
    Co: int
    training: bool = True
    Ci: int = 8
    N: int = 4
    H: int = 8
    W: int = 8
    groups: int = 2

    @property
    def name(self):
        return f"stage-{self.variant}-{self.Ci}-{self.Co}-{'train' if self.training else 'eval'}"


STAGE_CASES = ([StageCase(v, co) for v in ("plain", "pool", "head", "two") for co in (8, 12)]
               + [StageCase("im2col", co, Ci=2) for co in (8, 12)]
               + [StageCase("plain", co, training=False) for co in (8, 12)])


@dataclass(frozen=True)
class LoopCase:
    """ConvLSTMCell.forward called T times in a Python loop (one shared module, T uses, one backward)."""
    T: int = 3
    B: int = 1
    H: int = 4
    W: int = 4
    Cx: int = 8
    Hd: int = 8
    k: int = 3
    name: str = "cell-loop"


LOOP_CASE = LoopCase()


@dataclass(frozen=True)
class Head3Case:
    N: int = 2
    H: int = 8
    W: int = 8
    C: int = 16
    Co: int = 1
    name: str = "head3x3"


HEAD3_CASE = Head3Case()
FROZEN_SETS = [("weight",), ("bias",), ("weight", "bias")]


# ---------------------------------------------------------------------------------------------
# inputs (CPU, 16-bit-representable where the kernel reads 16 bits); ``scale``: the fp16 loss scale on every upstream gradient
# ---------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (1 << 31))


def _act(g, shape, valid, dtype, mul=0.8):
    t = torch.randn(*shape, generator=g) * mul
    t[..., valid:] = 0
    return r16(t, dtype)


def _away(g, shape, mul):
    """Gradients of magnitude >= 0.25 * mul: fp16 products and roundings stay clear of the subnormal range."""
    t = torch.randn(*shape, generator=g)
    return torch.sign(t) * (t.abs() + 0.25) * mul


def convt_inputs(c: ConvTCase, dtype, scale=1.0, seed=0):
    g = _gen(1, c.Ci, c.Co, seed)
    Cop = cpad(c.Co)
    du = _away(g, (c.N, 2 * c.h, 2 * c.w, Cop), scale)
    du[..., c.Co:] = 0
    return dict(x=_act(g, (c.N, c.h, c.w, cpad(c.Ci)), c.Ci, dtype), weight=torch.randn(c.Ci, c.Co, 2, 2, generator=g) * 0.2,
                bias=torch.randn(c.Co, generator=g) * 0.1, du=r16(du, dtype))


def outconv_inputs(c: OutConvCase, dtype, scale=1.0, seed=0):
    g = _gen(2, c.Ci, c.Co, seed)
    return dict(a=_act(g, (c.N, c.H, c.W, cpad(c.Ci)), c.Ci, dtype), weight=torch.randn(c.Co, c.Ci, 1, 1, generator=g) * 0.3,
                bias=torch.randn(c.Co, generator=g), dy=_away(g, (c.N, c.Co, c.H, c.W), scale))


def attn_inputs(c: AttnCase, dtype, scale=1.0, seed=0):
    g = _gen(3, c.k, seed)
    Cp = cpad(c.C)
    x = torch.randn(c.N, c.H, c.W, Cp, generator=g)
    x = r16(torch.sign(x) * (x.abs() + 0.25), dtype)
    dout = r16(_away(g, (c.N, c.H, c.W, Cp), scale), dtype)
    x[..., c.C:] = 0
    dout[..., c.C:] = 0
    return dict(x=x, weight=torch.randn(1, 2, c.k, c.k, generator=g) * (0.4 / c.k), dout=dout)


def head3_inputs(c: Head3Case, dtype, scale=1.0, seed=0):
    g = _gen(4, c.C, c.Co, seed)
    return dict(a=_act(g, (c.N, c.H, c.W, cpad(c.C)), c.C, dtype), weight=torch.randn(c.Co, c.C, 3, 3, generator=g) * (2.0 / (9 * c.C)) ** 0.5,
                bias=torch.randn(c.Co, generator=g) * 0.3, dy=_away(g, (c.N, c.Co, c.H, c.W), scale))


def stage_inputs(c: StageCase, dtype, scale=1.0, seed=0):
    """The dict of tests/test_gpu_conv_stage.py's _case (x, weight, bias, gamma, beta, head_w, head_b, da, dp, dy, Co) plus the
    variant's own sources: ``x1`` (6 x 6, 3 valid channels, with x0 keeping 5) for "two", ``x_nchw`` f32 for "im2col"."""
    g = _gen(5, c.Ci, c.Co, int(c.training), sum(map(ord, c.variant)), seed)
    Cop, Cip = cpad(c.Co), cpad(c.Ci)
    d = {"Co": c.Co, "gamma": torch.rand(c.Co, generator=g) + 0.5, "beta": torch.randn(c.Co, generator=g) * 0.2,
         "bias": torch.randn(c.Co, generator=g) * 0.1, "head_w": torch.randn(1, c.Co, 1, 1, generator=g) * 0.3,
         "head_b": torch.randn(1, generator=g), "weight": torch.randn(c.Co, c.Ci, 3, 3, generator=g) * 0.2}
    if c.variant == "two":
        d["x"] = _act(g, (c.N, c.H, c.W, Cip), 5, dtype).to(dtype)
        d["x1"] = _act(g, (c.N, c.H - 2, c.W - 2, 8), 3, dtype).to(dtype)
    elif c.variant == "im2col":
        d["x_nchw"] = r16(torch.randn(c.N, c.Ci, c.H, c.W, generator=g) * 0.8, dtype)
    else:
        d["x"] = _act(g, (c.N, c.H, c.W, Cip), c.Ci, dtype).to(dtype)
    for k, shape in (("da", (c.N, c.H, c.W, Cop)), ("dp", (c.N, c.H // 2, c.W // 2, Cop))):
        t = _away(g, shape, scale)
        t[..., c.Co:] = 0
        d[k] = t.to(dtype)
    d["dy"] = _away(g, (c.N, 1, c.H, c.W), scale)
    d["rm"], d["rv"] = torch.randn(c.Co, generator=g) * 0.1, torch.rand(c.Co, generator=g) + 0.5
    return d


def stage_sources(c: StageCase, d):
    """[(x NHWC, valid channels, offY, offX)] of the case, for conv3x3_wgrad_ref and stage_chain."""
    if c.variant == "two":
        return [(d["x"].float(), 5, 0, 0), (d["x1"].float(), 3, 1, 1)]
    if c.variant == "im2col":
        return [(d["x_nchw"].permute(0, 2, 3, 1).contiguous(), c.Ci, 0, 0)]
    return [(d["x"].float(), c.Ci, 0, 0)]


def stage_scale_grads(c: StageCase, d):
    """G64 of the pure f64 chain (for the scale of P only: the device's own dz carries 16-bit roundings)."""
    x = concat_sources(stage_sources(c, d), c.H, c.W)
    if c.variant == "head":
        r = stage_chain(x, d["weight"], d["bias"], d["gamma"], d["beta"], c.groups, True, None, head=(d["head_w"], d["head_b"]), dy=d["dy"])
    else:
        da = nchw(d["da"].float(), c.Co)
        if c.variant == "pool":          # the pooled output's gradient lands on one element of each window: same scale
            da = da + F.interpolate(nchw(d["dp"].float(), c.Co), scale_factor=2) * 0.25
        r = stage_chain(x, d["weight"], d["bias"], d["gamma"], d["beta"], c.groups, c.training, da, rm=d["rm"], rv=d["rv"])
    return r["grads"]


def loop_inputs(c: LoopCase, dtype, scale=1.0, seed=0):
    """f32 NCHW frames and upstream gradients of h_t (16-bit-representable), gate weight small enough for fp16's gate range."""
    g = _gen(6, c.T, c.Hd, seed)
    f16 = dtype == torch.float16
    fan = c.k * c.k * (c.Cx + c.Hd)
    return dict(xs=[r16(torch.randn(c.B, c.Cx, c.H, c.W, generator=g) * 0.8, dtype) for _ in range(c.T)],
                weight=torch.randn(4 * c.Hd, c.Cx + c.Hd, c.k, c.k, generator=g) * ((0.45 if f16 else 1.6) / fan ** 0.5),
                bias=torch.randn(4 * c.Hd, generator=g) * (0.1 if f16 else 0.3),
                dhs=[r16(_away(g, (c.B, c.Hd, c.H, c.W), scale), dtype) for _ in range(c.T)])
