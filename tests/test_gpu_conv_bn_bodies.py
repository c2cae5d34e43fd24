"""The convolution + BatchNorm + ReLU arithmetic of the two models, route against route: the one-node stage of TemporalUNetDualView
(ops.ConvBNReLU: one source, no bias, one group) against the decomposed encoder nodes of PretrainedTemporalUNet (resnet.EncConv,
stride 1 without a downsample, then resnet.BnRelu) on the same tensors; and the backward route of the two f32 heads
(ops.OutConv1x1, resnet.Head3x3), attached against returned and frozen subsets against the all-trainable run.

Both routes are the same launches with the same arguments, so every comparison is torch.equal under ops.deterministic(True), and the
launch records (LAUNCH_LOG and the PROFILE_HBM kinds with their byte counts) are equal as multisets.  The yardstick of each test is
the A route run twice from the same inputs, asserted bit-identical first (tests/test_gpu_conv_stage.py).  Shapes: n 2, 8 x 8,
24 -> 40 channels (K and N padded inside the panel; a per-tap kernel shape) and n 2, 16 x 16, 64 -> 64 (512 pixels: the 64-channel
shapes); the heads on the cases of tests/grad_route_cases.py.
"""
from collections import Counter

import pytest
import torch
import torch.nn as nn

import grad_route_cases as GC
from conftest import rel_l2
from test_gpu_conv_stage import _same

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_convlstm_amd import ops, resnet

DEV = "cuda"
N = 2
SHAPES = [(8, 8, 24, 40), (16, 16, 64, 64)]          # (H, W, Ci, Co)
DTYPES = [torch.bfloat16, torch.float16]
PARAMS = ("weight", "gamma", "beta")
MOM, EPS = 0.1, 1e-5


def _case(H, W, Ci, Co, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    Cip, Cop = ops.cpad(Ci), ops.cpad(Co)
    x = torch.randn(N, H, W, Cip, generator=g)
    x[..., Ci:] = 0
    da = torch.randn(N, H, W, Cop, generator=g)
    da[..., Co:] = 0
    return {"x": x.to(dtype), "da": da.to(dtype), "weight": torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5,
            "gamma": torch.rand(Co, generator=g) + 0.5, "beta": torch.randn(Co, generator=g) * 0.2,
            "rm": torch.randn(Co, generator=g) * 0.1, "rv": torch.rand(Co, generator=g) + 0.5, "Ci": Ci, "Co": Co}


def _records():
    """What has been launched since the records were last emptied, as a multiset."""
    rec = Counter(ops.LAUNCH_LOG) + Counter((k, nbytes) for k, nbytes, *_ in ops.PROFILE_HBM)
    ops.LAUNCH_LOG, ops.PROFILE_HBM = [], []
    return rec


def _run(c, route, mode, attach):
    """``route`` "stage": ConvBNReLU; "nodes": EncConv + BnRelu (under no_grad: the encoder's function that is not under autograd).
    ``mode``: "train", "eval_bwd" (running statistics with a backward pass) or "fold" (running statistics under no_grad).
    Returns the tensors and the (forward, backward) launch multisets."""
    training, grad = mode == "train", mode != "fold"
    x = c["x"].to(DEV).requires_grad_(grad)
    P = {k: c[k].to(DEV).requires_grad_(grad) for k in PARAMS}
    if attach and grad:
        for p in P.values():
            p.grad = torch.zeros_like(p)
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    ops.LAUNCH_LOG, ops.PROFILE_HBM = [], []
    try:
        with torch.set_grad_enabled(grad):
            if route == "stage":
                a = ops.ConvBNReLU.apply(x, None, P["weight"], None, P["gamma"], P["beta"], rm, rv, (c["Ci"],), (0, 0), 1, training, MOM, EPS,
                                         False)
            elif grad:
                z, par, _, _ = resnet.EncConv.apply(x, P["weight"], None, (P["gamma"], P["beta"], rm, rv, training, MOM, EPS), None, 1, False)
                a = resnet.BnRelu.apply(z, par, P["gamma"], P["beta"], training)
            else:
                conv, bn = nn.Conv2d(c["Ci"], c["Co"], 3, padding=1, bias=False), nn.BatchNorm2d(c["Co"], eps=EPS, momentum=MOM)
                conv.weight, bn.weight, bn.bias = (nn.Parameter(P[k], requires_grad=False) for k in PARAMS)
                bn.running_mean, bn.running_var = rm, rv
                pending = []
                a, par = resnet._conv_bn_forward(x, conv, bn.eval(), 1, pending, True, False)
                assert par is None and not pending, "running statistics under no_grad: the fold"
        ops.join_forward_side(x.device)
        torch.cuda.synchronize()
        fwd = _records()
        if grad:
            a.backward(c["da"].to(DEV))
            torch.cuda.synchronize()
        bwd = _records()
    finally:
        ops.LAUNCH_LOG = ops.PROFILE_HBM = None
    return {"a": a.detach(), "rm": rm, "rv": rv, "dx": x.grad, **{"d" + k: p.grad for k, p in P.items()}}, (fwd, bwd)


@pytest.mark.parametrize("attach", [False, True])
@pytest.mark.parametrize("mode", ["train", "eval_bwd", "fold"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,Ci,Co", SHAPES)
def test_stage_and_encoder_nodes_are_the_same_arithmetic(H, W, Ci, Co, dtype, mode, attach):
    """Activation, running statistics, dx, dweight, dgamma, dbeta and the forward and backward launch multisets of the one-node
    stage against those of EncConv + BnRelu."""
    c = _case(H, W, Ci, Co, dtype, seed=11)
    what = f"{H}x{W} {Ci}->{Co} {dtype} {mode} attach={attach}"
    with ops.deterministic(True):
        A, logA = _run(c, "stage", mode, attach)
        A2, logA2 = _run(c, "stage", mode, attach)
        _same(A, A2, what + ": stage, run to run")
        assert logA == logA2, what + ": stage launches, run to run"
        B, logB = _run(c, "nodes", mode, attach)
    _same(A, B, what + ": nodes against stage")
    assert logA[0] == logB[0], f"{what}: forward launches {logA[0]} / {logB[0]}"
    assert logA[1] == logB[1], f"{what}: backward launches {logA[1]} / {logB[1]}"
    assert float(A["a"].float().abs().max()) > 0
    assert sum(n for k, n in logA[0].items() if k[0] == "fwd") == 1, what
    if mode == "train":
        assert not torch.equal(A["rm"], c["rm"].to(DEV)) and not torch.equal(A["rv"], c["rv"].to(DEV)), what
    else:
        assert torch.equal(A["rm"], c["rm"].to(DEV)) and torch.equal(A["rv"], c["rv"].to(DEV)), what
    if mode == "fold":
        assert not logA[1] and all(A[k] is None for k in ("dx", "dweight", "dgamma", "dbeta")), what
        assert not any(k[0] in ("bn_apply_relu", "bn_bwd_reduce", "bn_bwd_apply") for k in logA[0]), what
    else:
        for k in ("dx", "dweight", "dgamma", "dbeta"):
            assert float(A[k].float().abs().max()) > 0, f"{what}: {k}"
        kinds = Counter(k[0] for k in logA[1].elements())
        assert (kinds["wgrad"], kinds["fwd"], kinds["bn_bwd_reduce"], kinds["bn_bwd_apply"]) == (1, 1, 1, 1), f"{what}: {logA[1]}"


# ---------------------------------------------------------------------------------------------
# the backward route of the two f32 heads
# ---------------------------------------------------------------------------------------------
MARK = 0.25          # fill of a frozen parameter's attached gradient buffer: must still be there afterwards
HEADS = {"outconv": lambda: (ops.OutConv1x1, GC.outconv_inputs, GC.OutConvCase(12, 3), "outconv_bwd"),
         "head3x3": lambda: (resnet.Head3x3, GC.head3_inputs, GC.HEAD3_CASE, "head3x3_bwd")}


def _run_head(cls, d, attach, frozen):
    a = d["a"].to(DEV).requires_grad_(True)
    P = {k: d[k].to(DEV).requires_grad_(k not in frozen) for k in ("weight", "bias")}
    if attach:
        for k, p in P.items():
            p.grad = torch.full_like(p, MARK) if k in frozen else torch.zeros_like(p)
    ops.LAUNCH_LOG, ops.PROFILE_HBM = [], []
    try:
        y = cls.apply(a, P["weight"], P["bias"])
        torch.cuda.synchronize()
        _records()
        y.backward(d["dy"].to(DEV))
        torch.cuda.synchronize()
        log = _records()
    finally:
        ops.LAUNCH_LOG = ops.PROFILE_HBM = None
    return {"y": y.detach(), "da": a.grad, **{"d" + k: p.grad for k, p in P.items()}}, log


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("head", sorted(HEADS))
def test_head_backward_routes(head, ordered, dtype):
    """OutConv1x1 and Head3x3, atomic and ordered: gradients written into attached buffers against gradients returned to autograd,
    and weight, bias or both frozen against the all-trainable run.  y and da bit-identical always, the parameter gradients
    bit-identical in ordered mode (atomic mode: f32 sums of N*H*W <= 128 terms in another order, 1e-5 of the norm); one
    ("reduce", kind) entry of the mode per backward pass, none with both frozen; Head3x3 alone records its backward launch with
    its byte count; a frozen parameter gets nothing and an attached buffer of it keeps its bits."""
    cls, inputs, case, kind = HEADS[head]()
    d = inputs(case, dtype)
    d["a"] = d["a"].to(dtype)          # (16-bit-representable f32 values)
    reduce = ("reduce", kind + ("_ordered" if ordered else ""))

    def same(A, B, what, keys):
        _same(A, B, what, keys=("y", "da"))
        for k in keys:
            if ordered:
                assert torch.equal(A[k], B[k]), f"{what}: {k}"
            else:
                e = rel_l2(A[k], B[k])
                print(f"[parity] {what}: {k} rel-L2 {e:.3e} (tol 1e-5)")
                assert e <= 1e-5, f"{what}: {k}"

    with ops.deterministic(ordered):
        ret, log = _run_head(cls, d, False, ())
        again, log2 = _run_head(cls, d, False, ())
        what = f"{head} ordered={ordered} {dtype}"
        same(ret, again, what + ": returned, run to run", ("dweight", "dbias"))
        assert log == log2 and log[reduce] == 1 and sum(n for k, n in log.items() if k[0] == "reduce") == 1, f"{what}: {log}"
        assert sum(n for k, n in log.items() if k[0] == "head3x3_bwd") == (1 if head == "head3x3" else 0), f"{what}: {log}"
        direct, logd = _run_head(cls, d, True, ())
        same(ret, direct, what + ": attached against returned", ("dweight", "dbias"))
        assert logd == log, f"{what}: attached launches {logd} / {log}"
        for k in ("da", "dweight", "dbias"):
            assert float(ret[k].float().abs().max()) > 0, k
        for frozen in GC.FROZEN_SETS:
            for attach in (False, True):
                frz, logf = _run_head(cls, d, attach, frozen)
                whatf = f"{what} frozen {frozen} attach={attach}"
                same(ret, frz, whatf, [k for k in ("dweight", "dbias") if k[1:] not in frozen])
                for k in frozen:
                    g = frz["d" + k]
                    if attach:
                        assert torch.equal(g, torch.full_like(g, MARK)), f"{whatf}: the attached buffer of frozen {k} was written"
                    else:
                        assert g is None, f"{whatf}: frozen {k} got a gradient"
                if len(frozen) == 2:
                    assert not any(k[0] in ("reduce", "head3x3_bwd") for k in logf), f"{whatf}: {logf}"
                else:
                    assert logf == log, f"{whatf}: launches {logf} / {log}"
