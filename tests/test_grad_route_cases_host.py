"""tests/grad_route_cases.py without a GPU: every f64 restatement equals PyTorch's own f64 modules to 1e-12, the checker accepts the
f32-rounded correct result and rejects each way of getting "+=" wrong with a message that names the parameter and the route."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import grad_route_cases as GC

F64 = torch.float64
BF16 = torch.bfloat16
B_SUM = 2e-6 + 4 * 2.0 ** -24          # a typical sum bound of the GPU tests (block_bound(4))


def close(a, b, what):
    e = float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))
    assert a.shape == b.shape and e <= 1e-12, f"{what}: {e:.3e}"


def module_grads(mod, x, g):
    mod = mod.double()
    mod.zero_grad()
    mod(x).backward(g)
    return {k: p.grad for k, p in mod.named_parameters()}


def terms_dominate(ref):
    for k, (G, T) in ref.items():
        assert bool((T >= G.abs() * (1 - 1e-12)).all()) and float(T.min()) > 0, k


# ---------------------------------------------------------------------------------------------
# the restatements against PyTorch's f64 modules
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GC.CONVT_CASES, ids=lambda c: c.name)
def test_convt_ref_equals_conv_transpose2d(c):
    d = GC.convt_inputs(c, BF16)
    m = nn.ConvTranspose2d(c.Ci, c.Co, 2, stride=2)
    want = module_grads(m, GC.nchw(d["x"], c.Ci), GC.nchw(d["du"], c.Co))
    ref = GC.convt_ref(d["x"], m.weight.shape, d["du"])
    close(ref["weight"][0], want["weight"], "weight")
    close(ref["bias"][0], want["bias"], "bias")
    terms_dominate(ref)


@pytest.mark.parametrize("c", GC.OUTCONV_CASES, ids=lambda c: c.name)
def test_outconv_ref_equals_conv2d_1x1(c):
    d = GC.outconv_inputs(c, BF16)
    m = nn.Conv2d(c.Ci, c.Co, 1)
    want = module_grads(m, GC.nchw(d["a"], c.Ci), d["dy"].double())
    ref = GC.outconv_ref(d["a"], m.weight.detach(), d["dy"])
    close(ref["weight"][0], want["weight"], "weight")
    close(ref["bias"][0], want["bias"], "bias")
    terms_dominate(ref)


@pytest.mark.parametrize("c", GC.ATTN_CASES, ids=lambda c: c.name)
def test_attn_ref_equals_autograd_through_conv2d_and_sigmoid(c):
    d = GC.attn_inputs(c, BF16)
    conv = nn.Conv2d(2, 1, c.k, padding=c.k // 2, bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(d["weight"].double())
    x = GC.nchw(d["x"], c.C)
    att = torch.sigmoid(conv(torch.cat((x.mean(1, keepdim=True), x.max(1, keepdim=True).values), 1)))
    (x * att).backward(GC.nchw(d["dout"], c.C))
    ref = GC.attn_ref(d["x"], d["weight"], c.C, d["dout"])
    close(ref["weight"][0], conv.weight.grad, "weight")
    terms_dominate(ref)


def test_head3x3_ref_equals_conv2d_3x3():
    c = GC.HEAD3_CASE
    d = GC.head3_inputs(c, BF16)
    m = nn.Conv2d(c.C, c.Co, 3, padding=1)
    want = module_grads(m, GC.nchw(d["a"], c.C), d["dy"].double())
    ref = GC.head3x3_ref(d["a"], m.weight.detach(), d["dy"])
    close(ref["weight"][0], want["weight"], "weight")
    close(ref["bias"][0], want["bias"], "bias")
    terms_dominate(ref)


@pytest.mark.parametrize("c", GC.STAGE_CASES, ids=lambda c: c.name)
def test_stage_chain_equals_conv2d_batchnorm2d_relu_and_the_pieces_equal_the_chain(c):
    """nn.Conv2d -> nn.BatchNorm2d applied per image group (or in eval mode on the running statistics) -> ReLU [-> nn.Conv2d 1x1] in
    f64 against stage_chain; then the piecewise references the GPU test feeds with the device's dz / sums / activation, fed with
    the chain's own, give the chain's gradients."""
    d = GC.stage_inputs(c, BF16)
    srcs = GC.stage_sources(c, d)
    x = GC.concat_sources(srcs, c.H, c.W)
    conv, bn, head = nn.Conv2d(x.shape[1], c.Co, 3, padding=1).double(), nn.BatchNorm2d(c.Co).double(), nn.Conv2d(c.Co, 1, 1).double()
    with torch.no_grad():
        for p, k in ((conv.weight, "weight"), (conv.bias, "bias"), (bn.weight, "gamma"), (bn.bias, "beta"), (head.weight, "head_w"),
                     (head.bias, "head_b"), (bn.running_mean, "rm"), (bn.running_var, "rv")):
            p.copy_(d[k].double())
    bn.train(c.training)
    G = c.groups if c.training else 1
    z = conv(x)
    a = torch.relu(torch.cat([bn(t) for t in z.chunk(G, 0)], 0))
    is_head = c.variant == "head"
    da = None if is_head else GC.nchw(d["da"].float(), c.Co)
    if is_head:
        head(a).backward(d["dy"].double())
        r = GC.stage_chain(x, d["weight"], d["bias"], d["gamma"], d["beta"], c.groups, True, None, head=(d["head_w"], d["head_b"]), dy=d["dy"])
        close(r["grads"]["head_w"], head.weight.grad, "head_w")
        close(r["grads"]["head_b"], head.bias.grad, "head_b")
    else:
        a.backward(da)
        r = GC.stage_chain(x, d["weight"], d["bias"], d["gamma"], d["beta"], c.groups, c.training, da, rm=d["rm"], rv=d["rv"])
    close(r["grads"]["weight"], conv.weight.grad, "weight")
    close(r["grads"]["gamma"], bn.weight.grad, "gamma")
    close(r["grads"]["beta"], bn.bias.grad, "beta")
    if c.training:          # a constant in front of batch statistics: cancellation noise of ~1e-16 x the terms
        assert float(r["grads"]["bias"].abs().max()) <= 1e-12 * float(r["dz"].abs().sum())
    else:
        close(r["grads"]["bias"], conv.bias.grad, "bias")
    # the pieces on the chain's own intermediates
    dz_nhwc = GC.pad_last(r["dz"].permute(0, 2, 3, 1), GC.cpad(c.Co))
    Gw, Tw = GC.conv3x3_wgrad_ref(srcs, dz_nhwc, c.Co)
    close(Gw, conv.weight.grad, "conv3x3_wgrad_ref")
    assert bool((Tw >= Gw.abs() * (1 - 1e-12)).all())
    pr = GC.bn_param_ref(GC.pad_last(r["sums"].permute(0, 2, 1), GC.cpad(c.Co)).permute(0, 2, 1), c.Co)
    close(pr["gamma"][0], bn.weight.grad, "bn_param_ref gamma")
    close(pr["beta"][0], bn.bias.grad, "bn_param_ref beta")
    if not c.training:
        close(GC.colsum_ref(dz_nhwc, c.Co)[0], conv.bias.grad, "colsum_ref")
    if is_head:
        hr = GC.fused_head_ref(GC.pad_last(r["a"].permute(0, 2, 3, 1), GC.cpad(c.Co)), d["dy"], c.Co)
        close(hr["head_w"][0], head.weight.grad, "fused_head_ref head_w")
        close(hr["head_b"][0], head.bias.grad, "fused_head_ref head_b")


def test_lstm_chain_equals_a_conv2d_cell_called_in_a_loop():
    c = GC.LOOP_CASE
    d = GC.loop_inputs(c, BF16)
    conv = nn.Conv2d(c.Cx + c.Hd, 4 * c.Hd, c.k, padding=c.k // 2).double()
    with torch.no_grad():
        conv.weight.copy_(d["weight"].double())
        conv.bias.copy_(d["bias"].double())
    h = torch.zeros(c.B, c.Hd, c.H, c.W, dtype=F64)
    cc, loss = torch.zeros_like(h), 0.0
    for t in range(c.T):          # train/unet.py:21-36
        cc_i, cc_f, cc_g, cc_o = torch.split(conv(torch.cat([d["xs"][t].double(), h], dim=1)), c.Hd, dim=1)
        cc = torch.sigmoid(cc_f) * cc + torch.sigmoid(cc_i) * torch.tanh(cc_g)
        h = torch.sigmoid(cc_o) * torch.tanh(cc)
        loss = loss + (h * d["dhs"][t].double()).sum()
    loss.backward()
    ref = GC.lstm_chain(d["xs"], d["weight"], d["bias"], c.Hd, d["dhs"])
    close(ref["weight"], conv.weight.grad, "weight")
    close(ref["bias"], conv.bias.grad, "bias")
    uses = GC.lstm_chain(d["xs"], d["weight"], d["bias"], c.Hd, d["dhs"], per_use=True)
    close(sum(u["weight"] for u in uses), conv.weight.grad, "sum of the uses")
    assert all(float(u["weight"].abs().max()) > 0 for u in uses)


# ---------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------
def convt_scene(seed=0):
    c = GC.CONVT_CASES[0]
    d = GC.convt_inputs(c, BF16, seed=seed)
    ref = GC.convt_ref(d["x"], d["weight"].shape, d["du"])
    return ref, GC.draw_P(ref, seed)


def f32(t):
    return t.double().float()


def test_checker_accepts_the_f32_rounded_correct_result():
    ref, P = convt_scene()
    ref_b, _ = convt_scene(seed=1)
    for k, (G, T) in ref.items():
        assert GC.check_param("host", k, "direct", f32(P[k].double() + G), P[k], [GC.Add(G, T, B_SUM)]) <= 1.0
        assert GC.check_param("host", k, "autograd", f32(G), None, [GC.Add(G, T, B_SUM)]) <= 1.0
        two = [GC.Add(G, T, B_SUM), GC.Add(*ref_b[k], B_SUM)]
        assert GC.check_param("host", k, "direct", f32(f32(P[k].double() + G).double() + ref_b[k][0]), P[k], two) <= 1.0
    GC.check_frozen("host", "weight", "direct", torch.full((3, 3), GC.MARK), True)
    GC.check_frozen("host", "weight", "autograd", None, False)


def rejected(name, route, got, P, adds, expect):
    with pytest.raises(GC.RouteError) as e:
        GC.check_param("host", name, route, got, P, adds)
    msg = str(e.value)
    print(f"[mutant] {msg}")
    assert name in msg and f"[{route} route]" in msg and expect in msg, msg


def test_checker_rejects_a_store_where_an_add_is_required():
    ref, P = convt_scene()
    for k, (G, T) in ref.items():
        rejected(k, "direct", f32(G), P[k], [GC.Add(G, T, B_SUM)], "stored instead of added")


def test_checker_rejects_P_added_twice():
    ref, P = convt_scene()
    for k, (G, T) in ref.items():
        rejected(k, "direct", f32(2 * P[k].double() + G), P[k], [GC.Add(G, T, B_SUM)], "P added twice")


def test_checker_rejects_P_dropped_for_the_bias_only():
    ref, P = convt_scene()
    G, T = ref["weight"]
    assert GC.check_param("host", "weight", "direct", f32(P["weight"].double() + G), P["weight"], [GC.Add(G, T, B_SUM)]) <= 1.0
    G, T = ref["bias"]
    rejected("bias", "autograd", f32(G), P["bias"], [GC.Add(G, T, B_SUM)], "stored instead of added")


def test_checker_rejects_a_dropped_second_use_of_a_shared_module():
    c = GC.LOOP_CASE
    d = GC.loop_inputs(c, BF16)
    uses = GC.lstm_chain(d["xs"], d["weight"], d["bias"], c.Hd, d["dhs"], per_use=True)
    tot = {k: sum(u[k] for u in uses) for k in ("weight", "bias")}
    P = GC.draw_P(tot, 3)
    for k in ("weight", "bias"):
        # T64 of a use: the host has no device dgates to expand; 16 x the rms of the use bounds its terms from above loosely
        adds = [GC.Add(u[k], u[k].abs() + 16 * u[k].pow(2).mean().sqrt(), B_SUM) for u in uses]
        assert GC.check_param("host", k, "direct", f32(P[k].double() + tot[k]), P[k], adds) <= 1.0
        rejected(k, "direct", f32(P[k].double() + uses[0][k] + uses[2][k]), P[k], adds, "addition 1 of 3 missing")


def test_checker_rejects_a_second_backward_pass_that_overwrites_the_first():
    ref_a, P = convt_scene()
    ref_b, _ = convt_scene(seed=1)
    for k in ref_a:
        adds = [GC.Add(*ref_a[k], B_SUM), GC.Add(*ref_b[k], B_SUM)]
        rejected(k, "direct", f32(P[k].double() + ref_b[k][0]), P[k], adds, "addition 0 of 2 missing")
        rejected(k, "autograd", f32(ref_b[k][0]), None, adds, "addition 0 of 2 missing")


def test_checker_rejects_a_written_frozen_buffer():
    ref, _ = convt_scene()
    G = ref["weight"][0]
    for got, attached in ((f32(GC.MARK + G), True), (f32(G), False), (None, True)):
        with pytest.raises(GC.RouteError) as e:
            GC.check_frozen("host", "weight", "direct", got, attached)
        assert "frozen weight" in str(e.value) and "[direct route]" in str(e.value)


def test_case_table_holds_the_route_decisions():
    assert [c.bias_direct for c in GC.CONVT_CASES] == [True, False]
    assert {(c.Ci, c.Co) for c in GC.OUTCONV_CASES} == {(8, 1), (8, 3), (12, 1), (12, 3)} and len(GC.ATTACH_SETS) == 3
    assert {c.k for c in GC.ATTN_CASES} == {3, 7}
    assert {c.variant for c in GC.STAGE_CASES} == {"plain", "pool", "head", "im2col", "two"}
    assert {c.Co for c in GC.STAGE_CASES} == {8, 12} and any(not c.training for c in GC.STAGE_CASES)
    c = GC.LOOP_CASE
    assert (c.T, c.B, c.H, c.W, c.Cx, c.Hd, c.k) == (3, 1, 4, 4, 8, 8, 3)
    # P: an O(1) share of the gradient, its ulp far below b * T64
    ref, P = convt_scene()
    for k, (G, T) in ref.items():
        ratio = float(P[k].double().pow(2).mean().sqrt() / G.pow(2).mean().sqrt())
        assert 0.5 <= ratio <= 2.0 and float((P[k].abs() * 2.0 ** -24).max()) < float((B_SUM * T).min())
