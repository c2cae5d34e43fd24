"""How a parameter gradient gets from a backward kernel into ``param.grad``: attached, accumulated, shared.

ops.py has two routes ("Where a gradient must be added, not stored"): the operator returns the gradient and autograd
accumulates it, or the kernel adds straight into an attached contiguous f32 ``.grad``.  Training always zeroes the flat gradient
buffer first, so in every model-level test the direct route adds onto zeros and a store in place of ``+=`` would pass.  Here the
buffers hold a random start value P (tests/grad_route_cases.py), two backward passes run without zeroing, one module is used
several times before one backward, and frozen neighbours keep a MARK fill:

    |grad - (P + sum G64)| <= sum_k b_k (T64_k + |buffer before addition k|)

with G64 / T64 the f64 gradient and the sum of the magnitudes of its terms, and b_k the bound the kernel behind that gradient holds
at the C ABI, imported from the suite that established it: the weight-gradient GEMM (test_gpu_wgrad_abi.coeff), block_bound(rows)
of test_gpu_deterministic.py for column sums, the 1x1 output convolution and the fused head's columns, check_sums' 2e-6 of
test_gpu_pointwise_abi.py for uclstm_bn_bwd_param_grads and (through test_gpu_boundary_abi.py) the attention weight,
(pixels + 2) * resnet_cases.U32 for Head3x3.  Gradients that are functions of tensors only the device holds (the BatchNorm stage's
dz and backward sums, the recurrence's dgates) take those stored tensors as the reference's inputs, as test_gpu_recurrence.py does.
fp16: every upstream gradient x 1024 and at least 0.25 x 1024 in magnitude.
"""
import contextlib
import datetime
import inspect
import os
from types import SimpleNamespace

import pytest
import torch

import grad_route_cases as GC
import recurrence_cases as RC
import resnet_cases as RNC
import test_gpu_boundary_abi as BA
import test_gpu_conv_stage as CS
import test_gpu_deterministic as TD
import test_gpu_pointwise_abi as PW
import test_gpu_wgrad_abi as WG
from conftest import per_tensor_grad_report

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops, resnet

L = RC.L
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
MODES = [False, True]          # ops.deterministic()
SWITCHES = ("DIRECT_GRADS", "ASYNC_WGRAD", "LAUNCH_LOG", "RECURRENCE_TRACE")
B_PARAM_GRADS = inspect.signature(PW.check_sums).parameters["tol"].default          # uclstm_bn_bwd_param_grads against f64
B_ATTN_DW = inspect.signature(BA.check_sums).parameters["tol"].default               # attention dw against f64
WORST = {}
tag = PW.tag


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """After the module's last test: the worst measured |err| / bound per operator, parameter and route (the DESIGN.md table; -s)."""
    yield
    for k, v in sorted(WORST.items()):
        print(f"[parity-summary] {k}: {v:.3e}")


@pytest.fixture(autouse=True)
def restore_switches():
    saved = {k: getattr(ops, k) for k in SWITCHES}
    hooks = (list(ops.USE_HOOKS), list(ops.GRAD_SIDE_HOOKS))
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.USE_HOOKS[:], ops.GRAD_SIDE_HOOKS[:] = hooks


def note(op, name, route, dtype, ratio):
    key = f"{op.split('-')[0]} [{route} route] {tag(dtype)}"          # the worst over the operator's parameters and variants
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def wgrad_b(M, log):
    """The weight-gradient GEMM's bound for M pixels and the slab count the launch took (LAUNCH_LOG: one "wgrad" entry)."""
    wg = [e for e in log if e[0] == "wgrad"]
    assert len(wg) == 1, f"weight-gradient launches {wg}"
    return WG.coeff(SimpleNamespace(M=M), int(wg[0][4]))


def reduce_kinds(log):
    return [e[1] for e in log if e[0] == "reduce"]


def colsum_b(pixels, Cp):
    return TD.block_bound(int(L.lib.uclstm_colsum_ordered_rows(pixels, Cp)))


@contextlib.contextmanager
def spy_backward(cls, returned):
    """What ``cls.backward`` hands to autograd, one tuple per backward call."""
    real = cls.backward

    def wrapped(ctx, *grads):
        out = real(ctx, *grads)
        returned.append(out if isinstance(out, tuple) else (out,))
        return out

    cls.backward = staticmethod(wrapped)
    try:
        yield
    finally:
        cls.backward = staticmethod(real)


def noncontiguous(P):
    """A non-contiguous f32 tensor of P's shape and values: permuted storage for a 4-D weight (where its size-1 axes leave that
    contiguous, and for a vector: every second element of a buffer twice as large).  None for a one-element tensor, which is
    contiguous whatever its strides."""
    if P.numel() == 1:
        return None
    g = torch.empty(P.shape[::-1], dtype=P.dtype, device=DEV).permute(*range(P.dim() - 1, -1, -1))
    if g.is_contiguous():
        g = torch.empty(P.shape + (2,), dtype=P.dtype, device=DEV)[..., 0]
    assert g.shape == P.shape and not g.is_contiguous()
    g.copy_(P)
    return g


# ---------------------------------------------------------------------------------------------
# the four operators whose parameter gradients are functions of the operator's inputs alone
# ---------------------------------------------------------------------------------------------
class Simple:
    def __init__(self, kind, c):
        self.kind, self.c, self.name = kind, c, c.name
        self.params = ("weight",) if kind == "attn" else ("weight", "bias")
        self.cls = {"convt": ops.ConvT2x2, "outconv": ops.OutConv1x1, "attn": ops.SpatialAttn, "head3": resnet.Head3x3}[kind]
        self.inputs = {"convt": GC.convt_inputs, "outconv": GC.outconv_inputs, "attn": GC.attn_inputs, "head3": GC.head3_inputs}[kind]
        self.act, self.up = {"convt": ("x", "du"), "outconv": ("a", "dy"), "attn": ("x", "dout"), "head3": ("a", "dy")}[kind]

    def apply(self, act, p):
        if self.kind == "attn":
            return self.cls.apply(act, p["weight"], self.c.C)
        return self.cls.apply(act, p["weight"], p["bias"])

    def refs(self, d):
        if self.kind == "convt":
            return GC.convt_ref(d["x"], d["weight"].shape, d["du"])
        if self.kind == "outconv":
            return GC.outconv_ref(d["a"], d["weight"], d["dy"])
        if self.kind == "attn":
            return GC.attn_ref(d["x"], d["weight"], self.c.C, d["dout"])
        return GC.head3x3_ref(d["a"], d["weight"], d["dy"])

    def bounds(self, log, weight_live=True):
        """{parameter: b} of one backward pass from its launch log."""
        c = self.c
        if self.kind == "convt":
            return {"weight": wgrad_b(c.N * c.h * c.w, log) if weight_live else 0.0, "bias": colsum_b(c.N * 4 * c.h * c.w, GC.cpad(c.Co))}
        if self.kind == "outconv":
            b = TD.block_bound(int(L.lib.uclstm_outconv_bwd_ordered_rows(c.N, c.H * c.W)))
            return {"weight": b, "bias": b}
        if self.kind == "attn":
            return {"weight": B_ATTN_DW}
        b = (c.N * c.H * c.W + 2) * RNC.U32
        return {"weight": b, "bias": b}

    def direct(self, attached, frozen):
        """{parameter: True where the kernel adds into the attached buffer itself} -- the route conditions of ops.py."""
        live = [k for k in self.params if k not in frozen]
        ok = {k: (k in attached and k in live and ops.DIRECT_GRADS and attached[k] == "contiguous") for k in self.params}
        if self.kind == "convt":
            return {"weight": "weight" in live and attached.get("weight") == "contiguous" and ops.ASYNC_WGRAD,
                    "bias": ok["bias"] and self.c.bias_direct}
        if self.kind == "attn":
            return {"weight": ok["weight"]}
        both = ok["weight"] and ok["bias"]          # direct_grad_pair: all or nothing
        return {"weight": both, "bias": both}

    def expected_reduces(self, det, frozen):
        """The "reduce" kinds of one backward pass."""
        sfx = "_ordered" if det else ""
        if self.kind == "convt":
            return [] if "bias" in frozen else ["colsum" + sfx]
        if self.kind == "outconv":
            return [] if len(frozen) == 2 else ["outconv_bwd" + sfx]
        if self.kind == "head3":
            return [] if len(frozen) == 2 else ["head3x3_bwd" + sfx]
        return []


def simple_run(op, dtype, passes, *, P=None, attach=(), frozen=(), strided=()):
    """Forward + backward of ``op`` once per entry of ``passes`` (input dicts) on ONE set of parameters, nothing zeroed in between.
    ``attach``: parameters that get ``.grad = P[name]`` beforehand (``strided``: as a non-contiguous tensor); a frozen parameter
    gets a MARK-filled buffer whenever anything is attached.  -> (grads, [launch log per pass], [tuple returned to autograd per pass],
    {name: "contiguous" | "strided"})."""
    first = passes[0]
    p = {k: first[k].to(DEV).requires_grad_(k not in frozen) for k in op.params}
    attached = {}
    for k in op.params:
        if k in frozen:
            if attach:
                p[k].grad = torch.full_like(p[k], GC.MARK)
        elif k in attach:
            g = noncontiguous(P[k].to(DEV)) if k in strided else None
            p[k].grad = g if g is not None else P[k].to(DEV).clone()
            attached[k] = "strided" if g is not None else "contiguous"
    logs, returned, states = [], [], []
    with spy_backward(op.cls, returned):
        for d in passes:
            # what each pass finds: after a first pass through autograd an unattached parameter owns a contiguous .grad too
            states.append({k: ("contiguous" if p[k].grad.is_contiguous() else "strided") for k in op.params
                           if k not in frozen and p[k].grad is not None})
            act = d[op.act].to(dtype).to(DEV).requires_grad_(True)
            up = d[op.up].to(DEV) if d[op.up].dtype == torch.float32 and op.up == "dy" else d[op.up].to(dtype).to(DEV)
            ops.LAUNCH_LOG = []
            op.apply(act, p).backward(up)
            torch.cuda.synchronize()
            logs.append(list(ops.LAUNCH_LOG))
            ops.LAUNCH_LOG = None
            assert act.grad is not None and bool(torch.isfinite(act.grad.float()).all())
    assert states[0] == attached
    return {k: p[k].grad for k in op.params}, logs, returned, states


def simple_check(op, dtype, det, passes, what, *, P=None, attach=(), frozen=(), strided=()):
    """Run, then hold every parameter to P + sum G64 (or to the frozen contract) and the launch log / autograd to the claimed route."""
    grads, logs, returned, states = simple_run(op, dtype, passes, P=P, attach=attach, frozen=frozen, strided=strided)
    refs = [op.refs(d) for d in passes]
    for i, log in enumerate(logs):
        direct = op.direct(states[i], frozen)
        assert reduce_kinds(log) == op.expected_reduces(det, frozen), f"{what}: pass {i} reduce launches {reduce_kinds(log)}"
        n_wgrad = len([e for e in log if e[0] == "wgrad"])
        assert n_wgrad == (1 if (op.kind == "convt" and "weight" not in frozen) else 0), f"{what}: {n_wgrad} weight-gradient launches"
        for j, k in enumerate(op.params):          # backward returns (d input, d weight, d bias | None)
            got_none = returned[i][1 + j] is None
            assert got_none == (direct[k] or k in frozen), \
                f"{what}: pass {i} handed autograd {'None' if got_none else 'a tensor'} for {k} (direct route claimed: {direct[k]})"
    bounds = [op.bounds(log, "weight" not in frozen) for log in logs]
    for k in op.params:
        route = "direct" if direct[k] else "autograd"
        if k in frozen:
            GC.check_frozen(what, k, route, grads[k], bool(attach))
            continue
        adds = [GC.Add(*r[k], b[k]) for r, b in zip(refs, bounds)]
        ratio = GC.check_param(what, k, route, grads[k], P[k] if k in attach else None, adds)
        print(f"[parity] {what} {tag(dtype)}: {k} [{route} route] worst |err| / bound {ratio:.3f}")
        note(op.kind, k, route, dtype, ratio)
    return grads


def simple_ops():
    return ([Simple("convt", c) for c in GC.CONVT_CASES] + [Simple("outconv", c) for c in GC.OUTCONV_CASES]
            + [Simple("attn", c) for c in GC.ATTN_CASES] + [Simple("head3", GC.HEAD3_CASE)])


def scaled(dtype):
    return PW.loss_scale(dtype)


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_attached_is_P_plus_G_and_unattached_is_G(dtype, det):
    """(a) and the attachment rows of (b): everything attached, nothing attached, weight only, bias only.  ConvT2x2 with Co = 12
    keeps the weight direct while its bias, whose buffer has not Cp elements, goes through autograd onto the attached P."""
    with ops.deterministic(det):
        for op in simple_ops():
            d = op.inputs(op.c, dtype, scaled(dtype))
            P = GC.draw_P(op.refs(d), 1)
            sets = [op.params, ()] + ([("weight",), ("bias",)] if len(op.params) == 2 else [])
            for attach in sets:
                simple_check(op, dtype, det, [d], f"{op.name} attached {attach or 'nothing'}", P=P, attach=attach)


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("fallback", ["strided", "DIRECT_GRADS off", "ASYNC_WGRAD off"])
def test_fallbacks_still_add_onto_P(fallback, dtype, det):
    """(b): a non-contiguous .grad of the right shape, ops.DIRECT_GRADS = False, ops.ASYNC_WGRAD = False: the operator must leave the
    direct route (autograd gets a tensor) and P + G must still come out."""
    if fallback == "DIRECT_GRADS off":
        ops.DIRECT_GRADS = False
    if fallback == "ASYNC_WGRAD off":
        ops.ASYNC_WGRAD = False
    with ops.deterministic(det):
        for op in simple_ops():
            d = op.inputs(op.c, dtype, scaled(dtype))
            P = GC.draw_P(op.refs(d), 2)
            if fallback == "strided":
                for k in op.params:          # one parameter at a time: its neighbour stays contiguous
                    simple_check(op, dtype, det, [d], f"{op.name} {k}.grad non-contiguous", P=P, attach=op.params, strided=(k,))
            else:
                simple_check(op, dtype, det, [d], f"{op.name} {fallback}", P=P, attach=op.params)


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_two_backward_passes_without_zeroing(dtype, det):
    """(c): forward / backward on inputs A, then on other inputs B, attached and not: P + G64_A + G64_B within the summed bounds; in
    deterministic mode the whole sequence twice is bit-identical."""
    with ops.deterministic(det):
        for op in simple_ops():
            dA, dB = op.inputs(op.c, dtype, scaled(dtype), seed=0), op.inputs(op.c, dtype, scaled(dtype), seed=1)
            dB = {**dB, **{k: dA[k] for k in op.params}}          # one set of parameters, other activations and upstream gradients
            P = GC.draw_P(op.refs(dA), 3)
            for attach in (op.params, ()):
                what = f"{op.name} passes A, B attached {attach or 'nothing'}"
                g1 = simple_check(op, dtype, det, [dA, dB], what, P=P, attach=attach)
                if det:
                    g2, _, _, _ = simple_run(op, dtype, [dA, dB], P=P, attach=attach)
                    assert all(torch.equal(g1[k], g2[k]) for k in op.params), f"{what}: not reproducible in deterministic mode"


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_frozen_neighbours(dtype, det):
    """(e): weight frozen, bias frozen, both frozen -- attached (MARK stays bit for bit) and not (.grad stays None); the other
    parameter's gradient is the unfrozen run's (bit for bit in deterministic mode); a fully frozen operator launches no
    weight-gradient GEMM and no reduction."""
    with ops.deterministic(det):
        for op in simple_ops():
            d = op.inputs(op.c, dtype, scaled(dtype))
            P = GC.draw_P(op.refs(d), 4)
            for attach in (op.params, ()):
                base = simple_check(op, dtype, det, [d], f"{op.name} unfrozen", P=P, attach=attach)
                for frozen in ([f for f in GC.FROZEN_SETS if set(f) <= set(op.params)]):
                    what = f"{op.name} frozen {frozen} attached {attach or 'nothing'}"
                    g = simple_check(op, dtype, det, [d], what, P=P, attach=attach, frozen=frozen)
                    if det:
                        for k in op.params:
                            if k not in frozen:
                                assert torch.equal(g[k], base[k]), f"{what}: {k} differs from the unfrozen run's"


# ---------------------------------------------------------------------------------------------
# ConvBNReLU through tests/test_gpu_conv_stage.py's _run
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def capture_stage(store):
    """The stage's device intermediates per backward pass: the conv output z, (scale, shift, mean, rstd), dz and the backward sums."""
    real = ops.ConvBNReLU._bn_backward

    def wrapped(ctx, z, par, head_w, head_b, da, dp):
        out = real(ctx, z, par, head_w, head_b, da, dp)
        store.append(dict(z=z, par=par, dz=out[0], sums=out[1], x0=ctx.saved_tensors[0], weight=ctx.saved_tensors[2]))
        return out

    ops.ConvBNReLU._bn_backward = staticmethod(wrapped)
    try:
        yield
    finally:
        ops.ConvBNReLU._bn_backward = staticmethod(real)


def stage_device_inputs(c, d, dtype):
    """The dict _run takes: the variant's own sources moved into its keys."""
    dd = dict(d)
    if c.variant == "im2col":
        with ops.compute_dtype(dtype):
            dd["x"] = ops.im2col_first(d["x_nchw"].to(DEV), False)
    if c.variant != "two":
        dd["x1"] = None
    kw = dict(variant=c.variant if c.variant in ("plain", "pool", "head") else "plain", training=c.training, groups=c.groups,
              c_valid={"two": (5, 3), "im2col": (c.Ci,)}.get(c.variant, (c.Ci,)), off=(1, 1) if c.variant == "two" else (0, 0),
              im2col=c.variant == "im2col")
    return dd, kw


def stage_adds(c, d, cap, log, dtype):
    """{parameter: Add} of one backward pass of the stage from the device's own z / dz / sums."""
    Co, Cop, pixels = c.Co, GC.cpad(c.Co), c.N * c.H * c.W
    G = c.groups if c.training else 1
    ppg = pixels // G
    dz = cap["dz"].float().cpu()
    out = {"weight": GC.Add(*GC.conv3x3_wgrad_ref(GC.stage_sources(c, d), dz, Co), wgrad_b(pixels, log))}
    for k, (g, t) in GC.bn_param_ref(cap["sums"].cpu(), Co).items():
        out[k] = GC.Add(g, t, B_PARAM_GRADS)
    if c.training:          # a constant in front of batch statistics: exactly += 0
        out["bias"] = GC.Add(torch.zeros(Co, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64), 0.0)
    else:
        out["bias"] = GC.Add(*GC.colsum_ref(dz, Co), colsum_b(pixels, Cop))
    if c.variant == "head":
        a = torch.empty_like(cap["z"])
        PW.call(L.kernels(dtype), "uclstm_bn_apply_relu", ops._p(cap["z"]), ops._p(a), ops._p(cap["par"][0]), ops._p(cap["par"][1]), pixels, ppg, Cop)
        b = TD.block_bound(int(L.lib.uclstm_bn_bwd_reduce_rows(pixels, ppg)))
        for k, (g, t) in GC.fused_head_ref(a.float().cpu(), d["dy"], Co).items():
            out[k] = GC.Add(g, t, b)
    return out


def stage_check(c, dtype, det, sets):
    """The stage once per attachment set of ``sets`` [(label, names to attach)]: every parameter against P + G64 from the device's
    own dz / sums, the launch log and what autograd received against the route conditions under the current switches."""
    d = GC.stage_inputs(c, dtype, scaled(dtype))
    P = GC.draw_P(GC.stage_scale_grads(c, d), 5)
    names = CS.PARAMS + (("head_w", "head_b") if c.variant == "head" else ())
    with ops.deterministic(det):
        dd, kw = stage_device_inputs(c, d, dtype)
        for label, attach in sets:
            attach = tuple(k for k in attach if k in names)
            what = f"{c.name} attached {label}" + ("" if ops.DIRECT_GRADS else ", DIRECT_GRADS off") + ("" if ops.ASYNC_WGRAD else ", ASYNC_WGRAD off")
            caps, returned, count = [], [], []
            with capture_stage(caps), spy_backward(ops.ConvBNReLU, returned):
                res, log = CS._run(dd, attach={k: P[k] for k in attach} if attach else False, count=count, **kw)
            adds = stage_adds(c, d, caps[0], log, dtype)
            bn_direct = ops.DIRECT_GRADS and "gamma" in attach and "beta" in attach
            head_direct = ops.DIRECT_GRADS and "head_w" in attach and "head_b" in attach
            direct = {"weight": ops.ASYNC_WGRAD and "weight" in attach, "gamma": bn_direct, "beta": bn_direct,
                      "bias": bn_direct and "bias" in attach, "head_w": head_direct, "head_b": head_direct}
            assert len(count) == (1 if bn_direct else 0), f"{what}: {len(count)} uclstm_bn_bwd_param_grads launches"
            sfx = "_ordered" if det else ""
            want = (["bn_head_bwd_reduce" + sfx] if c.variant == "head" else []) + ([] if c.training else ["colsum" + sfx])
            assert [k for k in reduce_kinds(log) if not k.startswith("unpack")] == want, f"{what}: reduce launches {reduce_kinds(log)}"
            slot = {"weight": 2, "bias": 3, "gamma": 4, "beta": 5, "head_w": 15, "head_b": 16}
            for k in names:
                route = "direct" if direct[k] else "autograd"
                assert (returned[0][slot[k]] is None) == direct[k], f"{what}: autograd got {returned[0][slot[k]]!r:.40} for {k} ({route} route claimed)"
                ratio = GC.check_param(what, k, route, res["d" + k], P[k] if k in attach else None, [adds[k]])
                print(f"[parity] {what} {tag(dtype)}: {k} [{route} route] worst |err| / bound {ratio:.3f}")
                note("stage-" + c.variant + ("" if c.training else "-eval"), k, route, dtype, ratio)


ALL_STAGE_PARAMS = CS.PARAMS + ("head_w", "head_b")


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("c", GC.STAGE_CASES, ids=lambda c: c.name)
def test_stage_attached_is_P_plus_G(c, dtype, det):
    """(a) for ConvBNReLU: plain / pool / fused head / im2col first layer / two sources, training and evaluation-mode BatchNorm;
    everything attached to P, nothing attached, and gamma attached without beta (uclstm_bn_bwd_param_grads needs both)."""
    stage_check(c, dtype, det, [("everything", ALL_STAGE_PARAMS), ("nothing", ()),
                                ("all but beta", tuple(k for k in ALL_STAGE_PARAMS if k != "beta"))])


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("switch", ["DIRECT_GRADS", "ASYNC_WGRAD"])
def test_stage_fallbacks_still_add_onto_P(switch, dtype, det):
    """(b) for ConvBNReLU: with ops.DIRECT_GRADS off only the weight stays direct, with ops.ASYNC_WGRAD off everything but the weight
    (and uclstm_bn_bwd_param_grads runs on the main stream); P + G either way.  Plain (Co 12), fused head (Co 8), frozen statistics."""
    setattr(ops, switch, False)
    for c in (GC.StageCase("plain", 12), GC.StageCase("head", 8), GC.StageCase("plain", 12, training=False)):
        stage_check(c, dtype, det, [("everything", ALL_STAGE_PARAMS)])


# ---------------------------------------------------------------------------------------------
# (d) one module, several uses, one backward
# ---------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, params):
        self.index = {id(p): k for k, p in params.items()}
        self.uses = {k: 0 for k in params}
        self.announced = {k: 0 for k in params}

    def use(self, p):
        if id(p) in self.index:
            self.uses[self.index[id(p)]] += 1

    def side(self, p):
        if id(p) in self.index:
            self.announced[self.index[id(p)]] += 1


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_convlstm_cell_called_three_times_in_a_loop(dtype, det):
    """The reference-style per-timestep loop: ConvLSTMCell.forward three times, the state handed on as f32 NCHW, one backward.  Weight
    and bias are attached to random P.  Each call is a ConvLSTMSeq of one step whose stored history (ops.RECURRENCE_TRACE) feeds
    the T = 3 sequence's f64 weight- and bias-gradient formulas (recurrence_cases.Ref.wgrad / bgrad over the three steps): three
    additions onto P, each under the weight-gradient GEMM's and the column sum's bound."""
    c = GC.LOOP_CASE
    d = GC.loop_inputs(c, dtype, scaled(dtype))
    tot = GC.lstm_chain(d["xs"], d["weight"].to(dtype).float(), d["bias"], c.Hd, d["dhs"])
    P = GC.draw_P(tot, 6)
    with ops.deterministic(det), ops.compute_dtype(dtype):
        cell = U.ConvLSTMCell(c.Cx, c.Hd, c.k).to(DEV)
        with torch.no_grad():
            cell.conv.weight.copy_(d["weight"])
            cell.conv.bias.copy_(d["bias"])
        params = {"weight": cell.conv.weight, "bias": cell.conv.bias}
        for k, p in params.items():
            p.grad = P[k].to(DEV).clone()
        probe = Probe(params)
        ops.USE_HOOKS.append(probe.use)
        ops.GRAD_SIDE_HOOKS.append(probe.side)
        ops.RECURRENCE_TRACE, ops.LAUNCH_LOG = trace, log = [], []
        state, loss = None, 0.0
        for t in range(c.T):
            h, state = cell(d["xs"][t].to(DEV), state)
            loss = loss + (h * d["dhs"][t].to(DEV)).sum()
        loss.backward()
        torch.cuda.synchronize()
    assert probe.uses == {"weight": c.T, "bias": c.T}, f"uses reported to USE_HOOKS: {probe.uses}"
    assert probe.announced == {"weight": c.T, "bias": c.T}, f"announcements in GRAD_SIDE_HOOKS: {probe.announced}"
    fwd, bwd = [e for e in trace if e[0] == "fwd"], [e for e in trace if e[0] == "bwd"]
    assert len(fwd) == c.T and len(bwd) == c.T
    if dtype == torch.float16:          # fp16 gates within [0.1, 0.9], no dgates near the subnormal range
        for e in fwd:
            g = e[3].double().reshape(-1, 4, GC.cpad(c.Hd))[..., :c.Hd]
            assert float(g[:, [0, 1, 3]].min()) >= 0.1 and float(g.abs().max()) <= 0.9, "fp16: a gate left [0.1, 0.9]"
    wg = [e for e in log if e[0] == "wgrad"]
    assert len(wg) == c.T and reduce_kinds(log).count("colsum_ordered" if det else "colsum") == c.T
    ref = RC.Ref(d["weight"].to(dtype).double(), d["bias"].double(), c.Hd, c.Cx, c.k)
    M, adds = c.B * c.H * c.W, {"weight": [], "bias": []}
    for i, t in enumerate(range(c.T - 1, -1, -1)):          # backward runs the calls last to first
        x_t = GC.pad_last(d["xs"][t].permute(0, 2, 3, 1), GC.cpad(c.Cx)).double()[None]
        h_prev, dg = fwd[t][1][:1].double().cpu(), bwd[i][1].double().cpu()
        if t == 0:
            assert not bool(h_prev.any())
        gw, tw, mapped = ref.wgrad(x_t, h_prev, dg)
        assert bool(mapped.all())
        adds["weight"].append(GC.Add(gw, tw, WG.coeff(SimpleNamespace(M=M), int(wg[i][4]))))
        adds["bias"].append(GC.Add(*ref.bgrad(dg), colsum_b(M, 4 * GC.cpad(c.Hd))))
    for k, p in params.items():
        ratio = GC.check_param(f"{c.name} attached", k, "direct", p.grad, P[k], adds[k])
        print(f"[parity] {c.name} {tag(dtype)} {'ordered' if det else 'atomic'}: {k} worst |err| / bound {ratio:.3f}")
        note("cellloop", k, "direct", dtype, ratio)
        # and against the T = 3 sequence's G64 from the pure f64 chain (lstm_chain, pinned to a Conv2d cell loop on the host).  What
        # separates the two is the 16-bit storage of the device's chain: per step h, the four gates, dh and the four dgates are
        # each rounded once (half a unit u16, relative), 10 roundings per step and 30 over the three steps that reach the first
        # use's gradient; first order, every one enters a gradient term at most once, so rel-L2 <= 30 u16 < 32 u16.  (A dropped or
        # doubled use is a third of the gradient or more.)
        rel = float((p.grad.double().cpu() - P[k].double() - tot[k]).norm() / tot[k].norm())
        print(f"[parity] {c.name} {tag(dtype)}: {k} rel-L2 against the pure f64 sequence {rel:.3e}")
        assert rel <= 32 * RC.u16(dtype), f"{c.name}: {k} is {rel:.3e} from the f64 sequence's gradient"


def doubleconv_twice(dtype, xs, sd, P):
    """One DoubleConv(8, 12) applied to the two inputs of ``xs`` under one backward; ``P``: start values to attach, or None."""
    dc = U.DoubleConv(8, 12).to(DEV).train()
    dc.load_state_dict(sd)
    params = dict(dc.named_parameters())
    if P is not None:
        for k, p in params.items():
            p.grad = P[k].to(DEV).clone()
    probe = Probe(params)
    ops.USE_HOOKS.append(probe.use)
    ops.GRAD_SIDE_HOOKS.append(probe.side)
    caps = []
    try:
        with capture_stage(caps):
            ops.LAUNCH_LOG = log = []
            outs = [dc.forward_nhwc(d["x"].to(dtype).to(DEV).requires_grad_(True), groups=2) for d in xs]
            ops.join_forward_side(outs[0].device)
            torch.autograd.backward(outs, [d["da"].to(DEV) for d in xs])
            torch.cuda.synchronize()
    finally:
        ops.LAUNCH_LOG = None
        ops.USE_HOOKS.remove(probe.use)
        ops.GRAD_SIDE_HOOKS.remove(probe.side)
    return params, probe, caps, log


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_one_doubleconv_applied_to_two_inputs_under_one_loss(dtype, det):
    """(d): one DoubleConv, two different inputs, one backward over both outputs: every parameter is used twice, announces itself
    twice and holds P + G_1 + G_2 -- each addition from the device's own input, dz and backward sums of that use.  First with
    nothing attached (autograd adds the two uses), which also gives rms(G) for the scale of P."""
    c = GC.StageCase("plain", 12)
    xs = [GC.stage_inputs(c, dtype, scaled(dtype), seed=s) for s in (0, 1)]
    torch.manual_seed(11)
    sd = {k: v.clone() for k, v in U.DoubleConv(8, 12).state_dict().items()}
    pixels, P = c.N * c.H * c.W, None
    with ops.deterministic(det):
        for attached in (False, True):
            params, probe, caps, log = doubleconv_twice(dtype, xs, sd, P)
            route = "direct" if attached else "autograd"
            assert all(v == 2 for v in probe.uses.values()), f"uses reported to USE_HOOKS: {probe.uses}"
            assert all(v == (2 if attached else 0) for v in probe.announced.values()), f"announcements ({route}): {probe.announced}"
            wg = [e for e in log if e[0] == "wgrad"]
            assert len(caps) == 4 and len(wg) == 4
            stage_of = {params["net.0.weight"].data_ptr(): ("net.0.", "net.1."), params["net.3.weight"].data_ptr(): ("net.3.", "net.4.")}
            adds = {k: [] for k in params}
            for cap, w in zip(caps, wg):          # the four stage backward passes in the order they ran, each followed by its GEMM
                conv, bn = stage_of[cap["weight"].data_ptr()]
                dz, ci = cap["dz"].float().cpu(), cap["weight"].shape[1]
                adds[conv + "weight"].append(GC.Add(*GC.conv3x3_wgrad_ref([(cap["x0"].float().cpu(), ci, 0, 0)], dz, 12),
                                                    WG.coeff(SimpleNamespace(M=pixels), int(w[4]))))
                pr = GC.bn_param_ref(cap["sums"].cpu(), 12)
                adds[bn + "weight"].append(GC.Add(*pr["gamma"], B_PARAM_GRADS))
                adds[bn + "bias"].append(GC.Add(*pr["beta"], B_PARAM_GRADS))
                z12 = torch.zeros(12, dtype=torch.float64)
                adds[conv + "bias"].append(GC.Add(z12, z12, 0.0))
            for k, p in params.items():
                assert len(adds[k]) == 2, k
                ratio = GC.check_param(f"DoubleConv on two inputs, {'P attached' if attached else 'nothing attached'}", k, route, p.grad,
                                       P[k] if attached else None, adds[k])
                print(f"[parity] DoubleConv on two inputs {tag(dtype)} [{route}]: {k} worst |err| / bound {ratio:.3f}")
                note("doubleconv twice", k, route, dtype, ratio)
            if not attached:
                P = GC.draw_P({k: p.grad.double().cpu() for k, p in params.items()}, 7)


# ---------------------------------------------------------------------------------------------
# (f) models under FusedAdamW / FlatParams: two micro-batches
# ---------------------------------------------------------------------------------------------
ACC_TOL = 1e-6          # "equal to f32 rounding" (test_config1_full_size_properties)
MODELS = ["unet", "resnet"]


def build_model(which, dtype):
    """(model, optimiser, [(x, y, mask) of micro-batch A, of B], loss-scaled backward)."""
    torch.manual_seed(21)
    if which == "unet":
        model = U.TemporalUNetDualView(1, 1, base_ch=8, lstm_layers=2, use_skip_lstm=True, use_attention=True).to(DEV).train()
        B, T, hw = 2, 2, 32
    else:
        model = U.PretrainedTemporalUNet(lstm_layers=1).to(DEV)
        model.load_state_dict(RNC.make_state(101, 1, 1), strict=True)
        model.train()
        B, T, hw = 1, 2, 64
    extra = dict(loss_scale=2.0 ** 10) if dtype == torch.float16 else {}
    opt = U.FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, **extra)
    batches = []
    for seed in (31, 32):
        d = U.SyntheticSequences(B, T, hw, hw, seed=seed, kind="uniform")
        batches.append((d.x, d.y, d.mask))
    return model, opt, batches


def micro_pass(model, opt, batch):
    x, y, mask = batch
    out = model(x)[0]
    y_pred = out.stacked if getattr(out, "stacked", None) is not None else (torch.stack(out, 1) if isinstance(out, (list, tuple)) else out)
    opt.scale_loss(U.compute_loss(y_pred, y, mask, True)).backward()


def accumulate(model, opt, buffers, passes, zero=True):
    """flat_g (host copy) after the given passes from the saved BatchNorm buffers, the flat buffer zeroed first."""
    with torch.no_grad():
        for k, b in model.named_buffers():
            b.copy_(buffers[k])
    if zero:
        opt.zero_grad()
    for p in passes:
        micro_pass(model, opt, p)
    torch.cuda.synchronize()
    return opt.flat.flat_g.detach().cpu().clone()


def compare_accumulated(what, model, opt, got, gA, gB):
    """Per tensor: rel-L2(got, gA + gB in f64) <= 1e-6 (conftest.per_tensor_grad_report's handling of analytically zero tensors); a
    tensor beyond that through cancellation is held element-wise to (rows + 1) 2^-24 (|gA| + |gB|) with rows = the planner's cap
    of partial rows (test_gpu_deterministic.ROWS_CAP).  Returns the worst rel-L2."""
    index = {id(p): k for k, p in model.named_parameters()}
    names = [index[id(p)] for p in opt.flat.params]
    cut = lambda flat: {k: flat[o:o + p.numel()].double() for k, o, p in zip(names, opt.flat.offsets, opt.flat.params)}
    G, A, B = cut(got), cut(gA), cut(gB)
    want = {k: A[k] + B[k] for k in names}
    norms = [float(want[k].norm()) for k in names]
    bad, rows, _ = per_tensor_grad_report(names, G, want, norms, [0.0] * len(names), floor=ACC_TOL, factor=1.0)
    worst = max(r[2] for r in rows if r[5] != "zero")
    print(f"[parity] {what}: {len(names)} tensors, worst rel-L2 of the accumulated buffer against gA + gB {worst:.3e} (<= {ACC_TOL:.0e}); "
          + ", ".join(f"{r[1]} {r[2]:.2e}" for r in rows[:3]))
    print(f"[parity] {what}: rel-L2 per tensor (analytically zero ones: the norm that arrived): "
          + ", ".join(f"{r[1]} {r[2]:.1e}{' (zero)' if r[5] == 'zero' else ''}" for r in rows))
    still = []
    for msg in bad:
        k = msg.split(":")[0]
        if k in want and "reference gradient is ~0" not in msg:
            lim = (TD.ROWS_CAP + 1) * 2.0 ** -24 * (A[k].abs() + B[k].abs()) + 1e-30
            e = float(((G[k] - want[k]).abs() / lim).max())
            print(f"[parity] {what}: {k} beyond {ACC_TOL:.0e} ({msg}); element-wise |err| / ((rows + 1) 2^-24 (|gA| + |gB|)) = {e:.3f}")
            if e <= 1.0:
                continue
        still.append(msg)
    assert not still, f"{what}: " + "; ".join(still)
    return worst


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("which", MODELS)
def test_model_gradient_accumulation_over_two_micro_batches(which, dtype, det):
    """(f): flat_g after A alone, after B alone and after A then B without zeroing in between, BatchNorm buffers restored before each
    run; the accumulated buffer per tensor against the f64 sum of the two single runs.  A store in one direct path loses gA of that
    tensor: rel-L2 >= 0.5."""
    with ops.deterministic(det), ops.compute_dtype(dtype):
        model, opt, (bA, bB) = build_model(which, dtype)
        buffers = {k: b.detach().clone() for k, b in model.named_buffers()}
        gA = accumulate(model, opt, buffers, [bA])
        gB = accumulate(model, opt, buffers, [bB])
        gAB = accumulate(model, opt, buffers, [bA, bB])
        assert float(gA.abs().max()) > 0 and float(gB.abs().max()) > 0 and not torch.equal(gA, gB)
        worst = compare_accumulated(f"{which} {tag(dtype)} {'ordered' if det else 'atomic'}", model, opt, gAB, gA, gB)
        WORST[f"model {which} accumulated rel-L2 {tag(dtype)} {'ordered' if det else 'atomic'}"] = worst
        if det:
            again = accumulate(model, opt, buffers, [bA, bB])
            assert torch.equal(again, gAB), "deterministic mode: the accumulated run is not reproducible"


# ---------------------------------------------------------------------------------------------
# (g) FlatDDP.no_sync() on the GPU, one rank
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def one_rank_group():
    """A one-rank gloo process group in this process (the shape of test_gpu_syncbn.py's gloo_one_rank)."""
    import torch.distributed as dist
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{32100 + os.getpid() % 1500}",
                                timeout=datetime.timedelta(seconds=60))
    group = dist.new_group(ranks=[dist.get_rank()], backend="gloo", timeout=datetime.timedelta(seconds=60))
    try:
        yield group
    finally:
        if created:
            dist.destroy_process_group()
        else:
            dist.destroy_process_group(group)


@pytest.mark.parametrize("det", MODES, ids=["atomic", "ordered"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_flatddp_no_sync_accumulates_and_releases_every_bucket_once(one_rank_group, dtype, det):
    """(g): zero_grad; reset(); pass A inside no_sync(); pass B outside; finalize().  The buffer is the plain accumulated one of (f);
    every bucket is launched exactly once and only after pass B has started; the use / announcement bookkeeping raises nothing; a
    second step of reset() + one pass releases its buckets early again (before finalize()): nothing leaked out of no_sync()."""
    with ops.deterministic(det), ops.compute_dtype(dtype):
        model, opt, (bA, bB) = build_model("unet", dtype)
        buffers = {k: b.detach().clone() for k, b in model.named_buffers()}
        gA, gB = accumulate(model, opt, buffers, [bA]), accumulate(model, opt, buffers, [bB])
        plain = accumulate(model, opt, buffers, [bA, bB])
        ddp = U.FlatDDP(model, opt.flat, bucket_mb=0.25, first_bucket_mb=0.05, process_group=one_rank_group)
        assert len(ddp.buckets) >= 3
        launched, phase = [], ["before"]
        real = ddp._launch

        def spy(bi):
            launched.append((bi, phase[0]))
            return real(bi)

        ddp._launch = spy

        def plain_step():
            """zero_grad + reset() + one pass + finalize(): how many buckets leave from the hooks, before finalize()."""
            launched.clear()
            opt.zero_grad()
            ddp.reset()
            phase[0] = "B"
            micro_pass(model, opt, bB)
            phase[0] = "finalize"
            ddp.finalize()
            torch.cuda.synchronize()
            assert sorted(bi for bi, _ in launched) == list(range(len(ddp.buckets))), f"bucket launches {launched}"
            return sum(1 for _, ph in launched if ph == "B")

        try:
            early0 = plain_step()
            assert early0 >= 1, "a plain step released no bucket from the hooks"
            launched.clear()
            with torch.no_grad():
                for k, b in model.named_buffers():
                    b.copy_(buffers[k])
            opt.zero_grad()
            ddp.reset()
            phase[0] = "A"
            with ddp.no_sync():
                micro_pass(model, opt, bA)
            phase[0] = "B"
            micro_pass(model, opt, bB)
            phase[0] = "finalize"
            ddp.finalize()
            torch.cuda.synchronize()
            got = opt.flat.flat_g.detach().cpu().clone()
            assert sorted(bi for bi, _ in launched) == list(range(len(ddp.buckets))), f"bucket launches {launched}"
            assert all(ph in ("B", "finalize") for _, ph in launched), f"a bucket left before pass B: {launched}"
            early = sum(1 for _, ph in launched if ph == "B")
            print(f"[parity] FlatDDP.no_sync {tag(dtype)}: {len(ddp.buckets)} buckets, {early} released during pass B, the rest in finalize()")
            if det:
                assert torch.equal(got, plain), "no_sync() + pass B differs from the plain accumulated buffer"
            else:
                compare_accumulated(f"FlatDDP.no_sync {tag(dtype)} atomic", model, opt, got, gA, gB)
            # the next step: reset() + one pass releases buckets from the hooks again
            early = plain_step()
            assert not any(ddp._unsynced_uses)
            assert early == early0, f"the step after no_sync() released {early} buckets from the hooks, a plain step {early0}"
        finally:
            ddp._launch = real
            ddp.remove_hooks()
