"""The conv3x3 + BatchNorm + ReLU stage (ops.ConvBNReLU) route against route: the branches of the stage that do the same
arithmetic by different launches must give the same bits.

Every comparison runs under ops.deterministic(True) and is torch.equal.  The yardstick of each test is the A route run twice from
the same inputs, asserted bit-identical first (as in test_frozen_convlstm_weights_launch_no_weight_gradient_and_leave_the_others_
alone): only then does "B differs from A" say something about B.  Shapes are the smallest that still have two BatchNorm groups,
more than one image per group and (Co = 12) padding channels: N 4, Ci 8, Co 16 / 12, 8 x 8 (7 x 9 for the odd map).
"""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

DEV = "cuda"
N, CI = 4, 8
PARAMS = ("weight", "bias", "gamma", "beta")
CONFIGS = [(16, torch.bfloat16), (12, torch.bfloat16), (16, torch.float16)]          # (Co, activation dtype)
MARK = 0.25          # fill of a frozen parameter's attached gradient buffer: must still be there afterwards


def _case(Co, H, W, dtype, seed=0):
    """CPU tensors of one stage: input, parameters, fused-head parameters and the upstream gradients of every variant."""
    g = torch.Generator().manual_seed(seed)
    Cop = ops.cpad(Co)

    def act(*shape, valid):
        t = torch.randn(*shape, generator=g)
        t[..., valid:] = 0                      # padding channels are exactly zero
        return t.to(dtype)

    return {"x": act(N, H, W, CI, valid=CI), "weight": torch.randn(Co, CI, 3, 3, generator=g) * 0.2,
            "bias": torch.randn(Co, generator=g) * 0.1, "gamma": torch.rand(Co, generator=g) + 0.5, "beta": torch.randn(Co, generator=g) * 0.2,
            "head_w": torch.randn(1, Co, 1, 1, generator=g) * 0.3, "head_b": torch.randn(1, generator=g),
            "da": act(N, H, W, Cop, valid=Co), "dp": act(N, H // 2, W // 2, Cop, valid=Co), "dy": torch.randn(N, 1, H, W, generator=g),
            "Co": Co}


def _run(c, *, attach=False, frozen=(), training=True, groups=2, variant="plain", skip_grad=True, count=None, c_valid=(CI,), off=(0, 0),
         im2col=False):
    """One forward + backward of the stage.  ``variant``: "plain", "pool" (the stage's own pooling), "pool_sep" (the stage, then
    MaxPool2Skip) or "head".  ``attach``: every parameter gets a contiguous f32 ``.grad`` before the run -- zeros for a trainable
    one (the backward kernels then add straight into it), MARK for a frozen one; a dict {name: start value} attaches a copy of the
    start value to the trainable parameters it names instead (tests/test_gpu_grad_routes.py).  ``c["x1"]`` with ``c_valid`` /
    ``off``: a second source; ``im2col``: ``c["x"]`` is the pre-gathered first-layer tensor.  Returns outputs, dx, the running
    statistics, every parameter's ``.grad`` and the LAUNCH_LOG of the run; ``count`` (a list) receives one entry per
    uclstm_bn_bwd_param_grads launch."""
    L = U._lib
    names = PARAMS + (("head_w", "head_b") if variant == "head" else ())
    x = c["x"].to(DEV).requires_grad_(True)
    x1 = c["x1"].to(DEV).requires_grad_(True) if c.get("x1") is not None else None
    P = {k: c[k].to(DEV).requires_grad_(k not in frozen) for k in names}
    if attach:
        for k, p in P.items():
            if k in frozen:
                p.grad = torch.full_like(p, MARK)
            elif not isinstance(attach, dict):
                p.grad = torch.zeros_like(p)
            elif k in attach:
                p.grad = attach[k].to(DEV).clone()
    rm, rv = torch.zeros(c["Co"], device=DEV), torch.ones(c["Co"], device=DEV)
    args = (x, x1, P["weight"], P["bias"], P["gamma"], P["beta"], rm, rv, tuple(c_valid), tuple(off), groups, training, 0.1, 1e-5, im2col)
    real = L.lib.uclstm_bn_bwd_param_grads

    def counted(*a):
        count.append(1)
        return real(*a)

    ops.LAUNCH_LOG = []
    if count is not None:
        L.lib.uclstm_bn_bwd_param_grads = counted
    try:
        a = p = None
        if variant == "head":
            y = ops.ConvBNReLU.apply(*args, P["head_w"], P["head_b"])
            outs, gos = [y], [c["dy"].to(DEV)]
        elif variant == "plain":
            a = ops.ConvBNReLU.apply(*args)
            outs, gos = [a], [c["da"].to(DEV)]
        else:
            if variant == "pool":
                a, p = ops.ConvBNReLU.apply(*args, None, None, True)
            else:
                p, a = ops.MaxPool2Skip.apply(ops.ConvBNReLU.apply(*args))
            outs, gos = ([a, p], [c["da"].to(DEV), c["dp"].to(DEV)]) if skip_grad else ([p], [c["dp"].to(DEV)])
        ops.join_forward_side(x.device)
        torch.autograd.backward(outs, gos)
        torch.cuda.synchronize()
        log = list(ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
        L.lib.uclstm_bn_bwd_param_grads = real
    res = {"dx": x.grad, "rm": rm, "rv": rv, **{"d" + k: q.grad for k, q in P.items()}}
    if variant == "head":
        res["y"] = y.detach()
    else:
        res["a"] = a.detach()
        if p is not None:
            res["p"] = p.detach()
    return res, log


def _same(A, B, what, keys=None):
    for k in (A.keys() if keys is None else keys):
        if A[k] is None or B[k] is None:
            assert A[k] is None and B[k] is None, f"{what}: {k} is None on one side only"
            continue
        if not torch.equal(A[k], B[k]):
            print(f"[parity] {what}: {k} differs, rel-L2 {rel_l2(A[k].float(), B[k].float()):.3e}")
        assert torch.equal(A[k], B[k]), f"{what}: {k}"


# ---------------------------------------------------------------------------------------------
# a. gradients returned to autograd against gradients written into the attached .grad buffers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Co,dtype", CONFIGS)
@pytest.mark.parametrize("variant,training", [("plain", True), ("pool", True), ("head", True), ("plain", False)])
def test_direct_gradients_equal_the_returned_ones(variant, training, Co, dtype):
    """Plain leaves (every gradient returned to autograd; the weight gradient unpacked on the main stream) against zero-filled f32
    .grad buffers attached beforehand (uclstm_bn_bwd_param_grads, the direct bias path, the weight gradient accumulated on the
    side stream; for the head, the reduction adding into head_w.grad / head_b.grad).  dgamma / dbeta: the kernel adds the groups
    in order from 0.f, and a sum of at most two f32 terms has one possible rounding.  training=False: frozen statistics, where
    the bias gradient is the column sum of dz, not zero."""
    c = _case(Co, 8, 8, dtype, seed=1)
    with ops.deterministic(True):
        for groups in (1, 2):
            what = f"{variant} training={training} Co={Co} {dtype} groups={groups}"
            count = []
            ret, _ = _run(c, training=training, groups=groups, variant=variant, count=count)
            again, _ = _run(c, training=training, groups=groups, variant=variant)
            _same(ret, again, what + ": returned route, run to run")
            assert not count, "plain leaves must not take the direct BatchNorm parameter-gradient kernel"
            direct, _ = _run(c, attach=True, training=training, groups=groups, variant=variant, count=count)
            assert len(count) == 1, "attached gradients must take the direct BatchNorm parameter-gradient kernel"
            _same(ret, direct, what + ": direct against returned")
            for k in ("dweight", "dgamma", "dbeta", "dx") + (("dhead_w", "dhead_b") if variant == "head" else ()):
                assert float(ret[k].abs().max()) > 0, k
            if training:
                assert float(ret["dbias"].abs().max()) == 0.0          # a constant in front of BatchNorm
            else:
                assert float(ret["dbias"].abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# b. partial freezing
# ---------------------------------------------------------------------------------------------
FROZEN_SETS = [(("gamma",), True), (("beta",), True), (("bias",), True), (("weight",), True), (("gamma", "beta"), True),
               (("bias",), False), (("weight",), False)]


@pytest.mark.parametrize("attach", [False, True])
@pytest.mark.parametrize("frozen,training", FROZEN_SETS)
def test_a_frozen_parameter_gets_nothing_and_leaves_the_others_alone(frozen, training, attach):
    """Any subset of the stage's parameters frozen: every still-trainable gradient and dx are bit-identical to the all-trainable
    run's; a frozen parameter's .grad stays None, an attached buffer keeps its bits; a frozen weight launches no weight-gradient
    GEMM; gamma and beta both frozen launch no uclstm_bn_bwd_param_grads."""
    for Co, dtype in CONFIGS[1:]:
        c = _case(Co, 8, 8, dtype, seed=2)
        what = f"frozen {frozen} training={training} attach={attach} Co={Co} {dtype}"
        with ops.deterministic(True):
            count = []
            base, log0 = _run(c, attach=attach, training=training, count=count)
            again, _ = _run(c, attach=attach, training=training)
            _same(base, again, what + ": all-trainable, run to run")
            assert len([e for e in log0 if e[0] == "wgrad"]) == 1 and len(count) == (1 if attach else 0)
            count = []
            frz, log = _run(c, attach=attach, frozen=frozen, training=training, count=count)
        live = [k for k in base if k[1:] not in frozen]
        _same(base, frz, what, keys=live)
        for k in frozen:
            g = frz["d" + k]
            if attach:
                assert torch.equal(g, torch.full_like(g, MARK)), f"{what}: the attached buffer of frozen {k} was written"
            else:
                assert g is None, f"{what}: frozen {k} got a gradient"
        assert len([e for e in log if e[0] == "wgrad"]) == (0 if "weight" in frozen else 1), what
        assert [e for e in log if e[0] == "fwd"] == [e for e in log0 if e[0] == "fwd"], what          # forward, input gradient
        both = "gamma" in frozen and "beta" in frozen
        one = ("gamma" in frozen) != ("beta" in frozen)
        assert len(count) == (0 if (both or one or not attach) else 1), f"{what}: {len(count)} bn_bwd_param_grads launches"


# ---------------------------------------------------------------------------------------------
# c. the stage's own unfused pooling against the stage followed by MaxPool2Skip
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip_grad", [True, False])
@pytest.mark.parametrize("H,W,training", [(7, 9, True), (8, 8, False)])
def test_unfused_pooling_inside_the_stage_equals_maxpool2skip_behind_it(H, W, training, skip_grad):
    """Odd maps (the fused kernels refuse) and evaluation-mode statistics with a backward pass are the two ways into the stage's
    stand-alone pooling branch.  A: ConvBNReLU.apply(..., pool=True); B: pool=False, then MaxPool2Skip.apply.  Same inputs, same
    two upstream gradients (or the skip output unused: da arrives as None): a, p, dx and every parameter gradient bit-identical."""
    for Co, dtype in CONFIGS:
        c = _case(Co, H, W, dtype, seed=3)
        what = f"unfused pool {H}x{W} training={training} skip gradient={skip_grad} Co={Co} {dtype}"
        with ops.deterministic(True):
            for attach in (False, True):
                A, log = _run(c, attach=attach, training=training, variant="pool", skip_grad=skip_grad)
                A2, _ = _run(c, attach=attach, training=training, variant="pool", skip_grad=skip_grad)
                _same(A, A2, what + ": stage's own pooling, run to run")
                B, _ = _run(c, attach=attach, training=training, variant="pool_sep", skip_grad=skip_grad)
                _same(A, B, what + f" attach={attach}")
                assert float(A["p"].float().abs().max()) > 0 and float(A["dx"].float().abs().max()) > 0


def test_even_training_map_takes_the_fused_pooling_and_equals_the_separate_kernels_in_a_and_p():
    """The other side of the decision: 8 x 8 in training mode pools inside the BatchNorm kernels; activation and pooled tensor are
    those of the separate kernels bit for bit (the gradients differ in f32 summation order:
    test_maxpool_fused_into_the_batchnorm_stage_matches_the_separate_kernels)."""
    c = _case(12, 8, 8, torch.bfloat16, seed=4)
    with ops.deterministic(True):
        A, _ = _run(c, variant="pool")
        B, _ = _run(c, variant="pool_sep")
    _same(A, B, "fused pool forward", keys=("a", "p", "rm", "rv"))


# ---------------------------------------------------------------------------------------------
# d. two sources against the zero-padded, concatenated single source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Co,dtype", CONFIGS)
def test_two_sources_equal_the_padded_concatenated_single_source(Co, dtype):
    """x1 (6 x 6, 3 valid channels of 8) centred at (1, 1) in x0 (8 x 8, 5 valid of 8) against one 8-channel source holding
    cat([x0, pad(x1)]).  a and dx0 bit-identical, the centre crop of the single-source dx is dx1; the weight gradient under the
    f32-accumulation tolerance of test_conv3x3_wgrad (2e-6: the K order of the two GEMMs differs)."""
    g = torch.Generator().manual_seed(5)
    c0, c1 = 5, 3
    x0 = torch.zeros(N, 8, 8, 8)
    x0[..., :c0] = torch.randn(N, 8, 8, c0, generator=g)
    x1 = torch.zeros(N, 6, 6, 8)
    x1[..., :c1] = torch.randn(N, 6, 6, c1, generator=g)
    xs = x0.clone()
    xs[:, 1:7, 1:7, c0:c0 + c1] = x1[..., :c1]
    c = _case(Co, 8, 8, dtype, seed=6)

    def run(two):
        srcs = [t.to(dtype).to(DEV).requires_grad_(True) for t in ((x0, x1) if two else (xs,))]
        P = {k: c[k].to(DEV).requires_grad_(True) for k in PARAMS}
        rm, rv = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
        a = ops.ConvBNReLU.apply(srcs[0], srcs[1] if two else None, P["weight"], P["bias"], P["gamma"], P["beta"], rm, rv,
                                 (c0, c1) if two else (c0 + c1,), (1, 1) if two else (0, 0), 2, True, 0.1, 1e-5, False)
        ops.join_forward_side(a.device)
        a.backward(c["da"].to(DEV))
        torch.cuda.synchronize()
        return {"a": a.detach(), "dx": [s.grad for s in srcs], "rm": rm, "rv": rv, **{"d" + k: q.grad for k, q in P.items()}}

    with ops.deterministic(True):
        two, again, one = run(True), run(True), run(False)
    what = f"two sources Co={Co} {dtype}"
    _same({**two, "dx0": two["dx"][0], "dx1": two["dx"][1], "dx": None}, {**again, "dx0": again["dx"][0], "dx1": again["dx"][1], "dx": None},
          what + ": run to run")
    dxs = one["dx"][0]
    _same(two, one, what, keys=("a",))          # (the f32 statistics themselves differ in summation order: 2e-7 in the running mean)
    assert torch.equal(two["dx"][0][..., :c0], dxs[..., :c0]) and not bool(two["dx"][0][..., c0:].any()), what + ": dx0"
    assert torch.equal(two["dx"][1][..., :c1], dxs[:, 1:7, 1:7, c0:c0 + c1]) and not bool(two["dx"][1][..., c1:].any()), what + ": dx1"
    assert float(two["dx"][1].float().abs().max()) > 0
    e = rel_l2(two["dweight"], one["dweight"])
    print(f"[parity] {what}: dweight rel-L2 {e:.3e} (tol 2e-6)")
    assert e <= 2e-6, what


# ---------------------------------------------------------------------------------------------
# DoubleConv: one call site for the three variants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "pool", "head"])
def test_doubleconv_stage_passes_pool_and_head_through(variant):
    """DoubleConv.forward_nhwc(head=..., pool=...) is two ConvBNReLU.apply calls, the second with the trailing optional
    arguments of its variant: outputs, running statistics, the bumped counters and every gradient bit-identical to the two calls
    written out."""
    torch.manual_seed(7)
    dc = U.DoubleConv(CI, 16).to(DEV).train()
    head = torch.nn.Conv2d(16, 1, 1).to(DEV)
    sd = {k: v.detach().clone() for k, v in dc.state_dict().items()}
    c = _case(16, 8, 8, torch.bfloat16, seed=8)
    res = []
    with ops.deterministic(True):
        for through_module in (True, True, False):
            dc.load_state_dict(sd)
            dc.zero_grad(set_to_none=True)
            head.zero_grad(set_to_none=True)
            x = c["x"].to(DEV).requires_grad_(True)
            conv0, bn0, conv1, bn1 = dc.net[0], dc.net[1], dc.net[3], dc.net[4]
            if through_module:
                out = dc.forward_nhwc(x, groups=2, head=head if variant == "head" else None, pool=variant == "pool")
            else:
                tail = {"plain": (), "pool": (None, None, True), "head": (head.weight, head.bias)}[variant]
                a0 = ops.ConvBNReLU.apply(x, None, conv0.weight, conv0.bias, bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var,
                                          (CI,), (0, 0), 2, True, bn0.momentum, bn0.eps, False)
                out = ops.ConvBNReLU.apply(a0, None, conv1.weight, conv1.bias, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var,
                                           (16,), (0, 0), 2, True, bn1.momentum, bn1.eps, False, *tail)
            ops.join_forward_side(x.device)
            outs = list(out) if variant == "pool" else [out]
            gos = {"plain": ["da"], "pool": ["da", "dp"], "head": ["dy"]}[variant]
            torch.autograd.backward(outs, [c[k].to(DEV) for k in gos])
            torch.cuda.synchronize()
            r = {f"out{i}": o.detach() for i, o in enumerate(outs)}
            r["dx"] = x.grad
            r.update({k: v.detach().clone() for k, v in dc.state_dict().items() if "num_batches" not in k})
            r.update({"d" + k: p.grad for k, p in list(dc.named_parameters()) + list(head.named_parameters(prefix="head"))})
            res.append(r)
            if through_module:
                assert int(bn0.num_batches_tracked) == 2 and int(bn1.num_batches_tracked) == 2
    _same(res[0], res[1], f"DoubleConv {variant}: run to run")
    _same(res[0], res[2], f"DoubleConv {variant}: module against the two calls written out")
    if variant != "head":
        assert res[0]["dhead.weight"] is None
