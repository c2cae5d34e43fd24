"""The ConvLSTM recurrence of ops.py (ConvLSTMSeq.forward / .backward, convlstm_group_forward + ConvLSTMSeqPre, convlstm_group_step,
the out= / direct inference forms) step by step against f64, in bf16 and fp16.

ops.RECURRENCE_TRACE hands out the tensors the recurrence stored per step (h_hist, c_hist, gates, dgates).  Every step's reference
takes the device's own stored inputs (tests/recurrence_cases.py), so each step is held to the bound its kernel holds at the C ABI:
the fused-cell bounds forward, the point-wise bound plus the propagated dc error backward, the STORE / weight-gradient / column-sum
bounds after the loop.  A wrong slot, buffer, slab count or slice is O(1) of these.  Every case asserts from KERNEL_LOG / LAUNCH_LOG
that the plan it is meant for ran (tests/test_recurrence_cases_host.py asserts the same plans without a GPU).

fp16: gradients x 1024 and at least 0.25 x 1024 in magnitude, gates in [0.1, 0.9], each asserted.
"""
import pytest
import torch

import recurrence_cases as RC
from recurrence_cases import RCase

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

L = RC.L
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
WORST = {}
SWITCHES = ("RECURRENCE_TRACE", "HOIST_X", "GROUP_LSTM", "ASYNC_WGRAD", "KERNEL_LOG", "LAUNCH_LOG", "split_k_factor")


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """After the module's last test: the worst measured |err| / bound per output and plan (the DESIGN.md table; run with -s)."""
    yield
    for (what, t), v in sorted(WORST.items()):
        print(f"[parity-summary] {what} {t}: {v:.3e}")


@pytest.fixture(autouse=True)
def restore_switches():
    saved = {k: getattr(ops, k) for k in SWITCHES}
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def report(name, dtype, plan_tag, worst):
    print(f"[parity] {name} {RC.tag(dtype)} ({plan_tag}): worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        key = (f"{k} [{plan_tag}]", RC.tag(dtype))
        WORST[key] = max(WORST.get(key, 0.0), v)
    assert all(v <= 1.0 for v in worst.values()), f"{name} {RC.tag(dtype)}: beyond the bound: { {k: round(v, 3) for k, v in worst.items() if v > 1} }"


def plan_tag(c, plan):
    f = "hoisted " if plan["hoist"] else ""
    f += f"{plan['fwd'][2]} slab(s) + point-wise" if plan["fwd"][1] > 1 else "fused cell"
    b = f"{plan['dh'][2]} f32 slabs" if plan["dh"][1] > 1 else "16-bit store"
    return f"k{c.k} {f} / {b}"


def assert_fp16_limits(dtype, c, inp, gates, chosen=("dh_all", "dc_T")):
    if dtype != torch.float16:
        return
    g = gates.double()[..., :c.Hd]
    assert float(g[..., [0, 1, 3], :].min()) >= 0.1 and float(g.abs().max()) <= 0.9, "fp16: a gate left [0.1, 0.9]"
    for k in chosen:
        if inp[k] is not None:
            v = inp[k].double().abs()
            assert float(v[v > 0].min()) >= 0.25 * 1024, f"fp16: {k} below 0.25 x the loss scale"


def device_run(c, dtype, inp=None, *, weight_grad=True, x_grad=True, attach=None, pre=None):
    """One ConvLSTMSeq.apply + torch.autograd.grad on the device with the trace and the logs on.  ``attach``: (P_w, P_b) f32
    tensors attached as weight.grad / bias.grad beforehand.  ``pre``: (h_hist, c_hist, gates) of an earlier forward, run
    through ConvLSTMSeqPre instead.  Returns a dict of host tensors, the logs and the device outputs."""
    inp = inp or RC.make_inputs(c, dtype)
    d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
    x, w, b, h0, c0 = d["x_all"].requires_grad_(x_grad), d["weight"].requires_grad_(weight_grad), d["bias"].requires_grad_(), d["h0"], d["c0"]
    if c.state:
        h0.requires_grad_()
        c0.requires_grad_()
    if attach is not None:
        w.grad, b.grad = attach[0].to(DEV).clone(), attach[1].to(DEV).clone()
    ops.RECURRENCE_TRACE, ops.KERNEL_LOG, ops.LAUNCH_LOG = trace, klog, llog = [], [], []
    ops.HOIST_X = c.hoist
    real = ops.split_k_factor
    if c.force:
        ops.split_k_factor = lambda *a, **k: c.force
    try:
        if pre is None:
            h_all, c_T = ops.ConvLSTMSeq.apply(x, h0, c0, w, b, c.Hd, c.Cx, True)
        else:
            h_all, c_T = ops.ConvLSTMSeqPre.apply(x, h0, c0, w, b, c.Hd, c.Cx, True, *pre)
            trace.append(("fwd",) + tuple(pre))
    finally:
        ops.split_k_factor = real
    n_fwd = len(klog)
    outs, gouts = [], []
    if d["dh_all"] is not None:
        outs, gouts = [h_all], [d["dh_all"]]
    if d["dc_T"] is not None:
        outs, gouts = outs + [c_T], gouts + [d["dc_T"]]
    ins = {"dx": x, "dh0": h0, "dc0": c0, "dW": w, "db": b}
    ins = {k: v for k, v in ins.items() if v is not None and v.requires_grad}
    grads = dict(zip(ins, torch.autograd.grad(outs, list(ins.values()), gouts, allow_unused=True)))
    ops.join_forward_side(x.device)
    torch.cuda.synchronize()
    if attach is not None:
        grads["dW"] = w.grad if grads["dW"] is None else grads["dW"]
        grads["db"] = b.grad if grads["db"] is None else grads["db"]
    (_, h_hist, c_hist, gates), (_, dgates) = trace[0], trace[-1]
    assert len(trace) == 2 and trace[-1][0] == "bwd"
    cpu = lambda t: None if t is None else t.detach().cpu()
    return dict(inp=inp, x_all=inp["x_all"], h_hist=cpu(h_hist), c_hist=cpu(c_hist), gates=cpu(gates), dgates=cpu(dgates),
                out={k: cpu(v) for k, v in grads.items()}, h_all=cpu(h_all), c_T=cpu(c_T), klog=klog, llog=llog, n_fwd=n_fwd,
                dev=(h_hist, c_hist, gates))


def assert_plan_ran(c, plan, run, need_h0, x_grad=True, weight_grad=True):
    """KERNEL_LOG / LAUNCH_LOG against the plan: forward launches per step, W_h^T launches per step, dx and weight-gradient launches."""
    Ktot, ks, nsl, fshape = plan["fwd"]
    exp = []
    for t in range(c.T):
        if plan["hoist"] and t == 0 and not c.state:
            continue                                           # the point-wise kernel alone
        exp.append((L.EPI_ATOMIC if ks > 1 else L.EPI_LSTM, fshape))
    fwd = run["klog"][:run["n_fwd"]]
    if plan["hoist"]:
        assert fwd[0][0] == L.EPI_ATOMIC, "no hoisted x GEMM"
        fwd = fwd[1:]
    assert fwd == exp, f"{c.name}: forward launches {fwd}, expected {exp}"
    _, kb, nb, bshape = plan["dh"]
    n_rec = c.T - 1 + int(need_h0)
    bwd = run["klog"][run["n_fwd"]:]
    assert bwd[:n_rec] == [(L.EPI_ATOMIC if kb > 1 else L.EPI_STORE, bshape)] * n_rec, f"{c.name}: W_h^T launches {bwd[:n_rec]}"
    assert (len(bwd) > n_rec) == x_grad, f"{c.name}: dx launches {bwd[n_rec:]}"
    wg = [e for e in run["llog"] if e[0] == "wgrad"]
    assert (len(wg) == 1) == weight_grad and len(wg) <= 1, f"{c.name}: weight-gradient launches {wg}"
    return int(wg[0][4]) if wg else 1


def check_run(c, dtype, plan, run, *, attach=None, name=None, chosen=("dh_all", "dc_T")):
    inp = run["inp"]
    ref = RC.Ref(inp["weight"].to(dtype).double(), inp["bias"].double(), c.Hd, c.Cx, c.k)
    zero_c0 = inp["c0"] is None
    assert_fp16_limits(dtype, c, inp, run["gates"], chosen)
    worst = RC.check_forward(c, dtype, ref, RC.fwd_coeffs(c, plan, zero_c0), run["x_all"], run["h_hist"], run["c_hist"], run["gates"], zero_c0)
    worst.update(RC.check_backward(c, dtype, ref, plan, x_all=run["x_all"], h_hist=run["h_hist"], c_hist=run["c_hist"], gates=run["gates"],
                                   dgates=run["dgates"], dh_all=inp["dh_all"], dc_T=inp["dc_T"], has_c0=not zero_c0, out=run["out"],
                                   wgrad_splits=run.get("splits", 1), base_w=None if attach is None else attach[0],
                                   base_b=None if attach is None else attach[1]))
    report(name or c.name, dtype, plan_tag(c, plan), worst)
    return worst


# ---------------------------------------------------------------------------------------------
# 1. every case of the table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_recurrence_step_by_step_against_f64(name, dtype):
    """ConvLSTMSeq.apply + autograd.grad with chosen grad_outputs: every stored step and every output inside its bound, the pad
    channels exactly 0, the intended plan in the logs, and the outputs the function returns are the last history slots."""
    c = RC.BY_NAME[name]
    plan = RC.plan_of(c)
    run = device_run(c, dtype)
    run["splits"] = assert_plan_ran(c, plan, run, need_h0=c.state)
    assert torch.equal(run["h_all"], run["h_hist"][1:]) and torch.equal(run["c_T"], run["c_hist"][c.T])
    worst = check_run(c, dtype, plan, run)
    want = {"c", "h", "gates", "dgates", "dx", "dW", "db"} | ({"dh0", "dc0"} if c.state else set())
    assert want <= set(worst), f"{name}: outputs not produced: {want - set(worst)}"


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_trace_switch_changes_no_launch_and_no_bit(dtype):
    """RECURRENCE_TRACE = None (the default) against a list: the same launches in the logs, the same bits in every result, and the
    entries are the stored tensors themselves."""
    c = RC.BY_NAME["A-state"]
    inp = RC.make_inputs(c, dtype)

    def once(trace):
        d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
        leaves = [d[k].requires_grad_() for k in ("x_all", "h0", "c0", "weight", "bias")]
        ops.RECURRENCE_TRACE, ops.KERNEL_LOG, ops.LAUNCH_LOG = trace, [], []
        ops.HOIST_X = False
        h_all, c_T = ops.ConvLSTMSeq.apply(*leaves, c.Hd, c.Cx, True)
        grads = torch.autograd.grad([h_all, c_T], leaves, [d["dh_all"], d["dc_T"]])
        torch.cuda.synchronize()
        return [h_all, c_T] + list(grads), ops.KERNEL_LOG, ops.LAUNCH_LOG

    off, k0, l0 = once(None)
    trace = []
    on, k1, l1 = once(trace)
    assert k0 == k1 and l0 == l1 and len(k0) > 0 and len(l0) > 0
    assert all(torch.equal(a, b) for a, b in zip(off, on))
    assert [e[0] for e in trace] == ["fwd", "bwd"] and trace[0][1][1:].data_ptr() == on[0].data_ptr()


# ---------------------------------------------------------------------------------------------
# 2. hoisted forward, shared backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
@pytest.mark.parametrize("name", ["A-hoist-state", "S-hoist"])
def test_backward_of_a_hoisted_forward_equals_the_unhoisted_backward(name, dtype):
    """The backward pass does not depend on how the forward pass was computed: fed the hoisted run's saved tensors through
    ConvLSTMSeqPre with HOIST_X off, every gradient is bit-identical."""
    c = RC.BY_NAME[name]
    a = device_run(c, dtype)
    plain = RCase(**{**c.__dict__, "hoist": False, "force": 0})
    b = device_run(plain, dtype, inp=a["inp"], pre=a["dev"])
    assert set(a["out"]) == set(b["out"])
    for k in a["out"]:
        assert torch.equal(a["out"][k], b["out"][k]), f"{name}: {k} differs"
    assert torch.equal(a["dgates"], b["dgates"])


# ---------------------------------------------------------------------------------------------
# 3. frozen weight, x without gradient, both weight-gradient routes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_frozen_weight_and_x_without_gradient_launch_less_and_change_nothing(dtype):
    c = RC.BY_NAME["A-state"]
    plan = RC.plan_of(c)
    full = device_run(c, dtype)
    assert_plan_ran(c, plan, full, need_h0=True)
    frozen = device_run(c, dtype, weight_grad=False)
    assert_plan_ran(c, plan, frozen, need_h0=True, weight_grad=False)
    assert "dW" not in frozen["out"] and not any(e[0] == "wgrad" for e in frozen["llog"])
    no_x = device_run(c, dtype, x_grad=False)
    assert_plan_ran(c, plan, no_x, need_h0=True, x_grad=False)
    for other in (frozen, no_x):
        for k, v in other["out"].items():
            assert torch.equal(v, full["out"][k]), f"{k} changes when another gradient is not asked for"
        assert torch.equal(other["dgates"], full["dgates"])


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
@pytest.mark.parametrize("name", ["A-state", "P5"])
def test_weight_gradient_accumulated_on_the_side_stream(name, dtype):
    """A pre-attached random f32 weight.grad / bias.grad: autograd gets None for the weight, the side stream adds dW onto P, and
    after the scheduled join the result is P + dW within the weight-gradient bound (Hd_p == Hd: the bias sums go into bias.grad
    too; Hd_p != Hd: they are returned)."""
    c = RC.BY_NAME[name]
    plan = RC.plan_of(c)
    torch.manual_seed(3)
    S = RC.loss_scale(dtype)
    P = (torch.randn(4 * c.Hd, c.Cx + c.Hd, c.k, c.k) * S, torch.randn(4 * c.Hd) * S)
    ops.ASYNC_WGRAD = True
    ref_run = device_run(c, dtype)
    assert ref_run["out"]["dW"] is not None                      # returned by autograd when nothing is attached
    inp = RC.make_inputs(c, dtype)
    d = device_run(c, dtype, inp=inp, attach=P)
    d["splits"] = assert_plan_ran(c, plan, d, need_h0=True)
    direct_bias = c.Hdp == c.Hd
    attach = (P[0], P[1] if direct_bias else None)
    if not direct_bias:
        assert not torch.equal(d["out"]["db"], P[1])
    check_run(c, dtype, plan, d, attach=attach, name=name + " accumulate")
    for k in ("dx", "dh0", "dc0"):
        assert torch.equal(d["out"][k], ref_run["out"][k])


# ---------------------------------------------------------------------------------------------
# 4. group forward
# ---------------------------------------------------------------------------------------------
GROUP = [RCase("G-64-64", 3, 1, 16, 16, 64, 64), RCase("G-128-64", 3, 1, 16, 16, 128, 64, state=True, dc_T=True),
         RCase("G-64-128", 3, 1, 8, 32, 64, 128, dc_T=True)]


def group_members(dtype, cases):
    out = []
    for c in cases:
        inp = RC.make_inputs(c, dtype)
        d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
        d["x_all"].requires_grad_()
        d["weight"].requires_grad_()
        d["bias"].requires_grad_()
        if c.state:
            d["h0"].requires_grad_()
            d["c0"].requires_grad_()
        out.append((inp, d, (d["x_all"], d["h0"], d["c0"], d["weight"], d["bias"], c.Hd, c.Cx)))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_group_forward_step_by_step_against_f64(dtype):
    """Three unlike members through convlstm_group_ok, convlstm_group_forward and ConvLSTMSeqPre: every member's every step inside
    the forward bound with the K-range count plan_group_ksplit chose, every member's backward as for a single sequence."""
    ops.GROUP_LSTM, ops.HOIST_X = True, False
    ms = group_members(dtype, GROUP)
    members = [m[2] for m in ms]
    assert ops.convlstm_group_ok(members)
    ksplits = ops.plan_group_ksplit([(((ops.lstm_pack_desc(c.Hd, c.Cx, 3).N + 127) // 128) * (c.pixels // 256),
                                      ops.lstm_pack_desc(c.Hd, c.Cx, 3).Ktot // (64 * 9)) for c in GROUP])
    ops.RECURRENCE_TRACE, ops.KERNEL_LOG = trace, klog = [], []
    res = ops.convlstm_group_forward(members, True)
    assert [e[0] for e in trace] == ["fwd"] * 3 and all(trace[i][1] is res[i][0] and trace[i][3] is res[i][2] for i in range(3))
    assert klog == [(L.EPI_ATOMIC if ks > 1 else L.EPI_LSTM, 2) for ks in ksplits] * 3, f"group launches {klog}"
    ops.KERNEL_LOG = None
    for i, (c, (inp, d, mem)) in enumerate(zip(GROUP, ms)):
        plan = RC.plan_of(c)
        pd = ops.lstm_pack_desc(c.Hd, c.Cx, 3)
        plan["fwd"] = (pd.Ktot, ksplits[i], ops.ksplit_used(pd.Ktot, ksplits[i], 3) if ksplits[i] > 1 else 0, 2)
        run = device_run(c, dtype, inp=inp, pre=res[i])
        run["splits"] = next(int(e[4]) for e in run["llog"] if e[0] == "wgrad")
        assert torch.equal(run["h_all"], run["h_hist"][1:]) and torch.equal(run["c_T"], run["c_hist"][c.T])
        check_run(c, dtype, plan, run, name=f"group member {c.name} ({ksplits[i]} K ranges)")


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_group_refuses_unlike_members(dtype):
    ops.GROUP_LSTM = True
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    ms = [m[2] for m in group_members(dtype, GROUP)]
    assert ops.convlstm_group_ok(ms)
    odd_dtype = group_members(other, [GROUP[0]])[0][2]
    assert not ops.convlstm_group_ok(ms + [odd_dtype])
    odd_T = group_members(dtype, [RCase("G-T2", 2, 1, 16, 16, 64, 64)])[0][2]
    assert not ops.convlstm_group_ok(ms + [odd_T])


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_group_step_against_f64_and_its_refusals(dtype):
    """convlstm_group_step on the three members: each new state inside the forward bound of the f64 cell on its inputs; a member
    without c_prev or with h_out aliasing h_prev makes it return False with nothing written."""
    ops.GROUP_LSTM = True
    cases = [RCase(**{**c.__dict__, "T": 1, "state": True}) for c in GROUP]
    ksplits = ops.plan_group_ksplit([(((ops.lstm_pack_desc(c.Hd, c.Cx, 3).N + 127) // 128) * (c.pixels // 256),
                                      ops.lstm_pack_desc(c.Hd, c.Cx, 3).Ktot // (64 * 9)) for c in cases])
    inps = [RC.make_inputs(c, dtype) for c in cases]

    def members(mutate=None):
        ms, outs = [], []
        for i, (c, inp) in enumerate(zip(cases, inps)):
            d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
            h_out = torch.full_like(d["h0"], float("nan"))
            c_out = torch.full_like(d["c0"], float("nan"))
            c_prev = None if (mutate == "no_c_prev" and i == 1) else d["c0"]
            ms.append((d["x_all"][0], d["h0"], c_prev, d["h0"] if (mutate == "alias" and i == 2) else h_out, c_out, d["weight"], d["bias"],
                       c.Hd, c.Cx))
            outs.append((h_out, c_out, d["h0"]))
        return ms, outs

    with torch.no_grad():
        for mutate in ("no_c_prev", "alias"):
            ms, outs = members(mutate)
            before = [o[2].clone() for o in outs]
            assert ops.convlstm_group_step(ms) is False
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(o[0]).all()) and bool(torch.isnan(o[1]).all()) for o in outs), f"{mutate}: something was written"
            assert all(torch.equal(o[2], b) for o, b in zip(outs, before))
        ms, outs = members()
        assert ops.convlstm_group_step(ms) is True
        torch.cuda.synchronize()
    for c, inp, (h_out, c_out, _), ks in zip(cases, inps, outs, ksplits):
        ref = RC.Ref(inp["weight"].to(dtype).double(), inp["bias"].double(), c.Hd, c.Cx, 3)
        pd = ops.lstm_pack_desc(c.Hd, c.Cx, 3)
        worst = RC.check_forward(c, dtype, ref, [RC.f32_coeff(pd.Ktot, ks)], inp["x_all"], torch.stack((inp["h0"], h_out.cpu())),
                                 torch.stack((inp["c0"], c_out.cpu())), None, False)
        worst.pop("gates")
        report(f"group step {c.name}", dtype, f"group step, {ks} K range(s)", worst)


def group_ksplits(cases):
    return ops.plan_group_ksplit([(((ops.lstm_pack_desc(c.Hd, c.Cx, 3).N + 127) // 128) * (c.pixels // 256),
                                   ops.lstm_pack_desc(c.Hd, c.Cx, 3).Ktot // (64 * 9)) for c in cases])


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_single_sequence_equals_its_group_member_bit_for_bit(dtype):
    """A group member is by construction a patch-shape launch on its own: ConvLSTMSeq with the member's planned K-range count stores
    the same bits in every slot of h_hist, c_hist and gates as convlstm_group_forward, through kernel shape 2 with the planned epilogue."""
    ops.GROUP_LSTM, ops.HOIST_X = True, False
    members = [m[2] for m in group_members(dtype, GROUP)]
    ksplits = group_ksplits(GROUP)
    with torch.no_grad():
        ops.RECURRENCE_TRACE = grouped = []
        ops.convlstm_group_forward(members, True)
        assert [e[0] for e in grouped] == ["fwd"] * 3
        for c, mem, ks, (_, h_g, c_g, g_g) in zip(GROUP, members, ksplits, grouped):
            ops.RECURRENCE_TRACE, ops.KERNEL_LOG = single, klog = [], []
            ops.split_k_factor = lambda *a, _ks=ks, **k: _ks
            ops.ConvLSTMSeq.apply(*mem, True)
            assert klog == [(L.EPI_ATOMIC if ks > 1 else L.EPI_LSTM, 2)] * c.T, f"{c.name}: single launches {klog}"
            (_, h_s, c_s, g_s), = single
            torch.cuda.synchronize()
            zero_c0 = mem[2] is None                                 # slot 0 of c_hist is never written nor read for a zero cell state
            assert torch.equal(h_s, h_g), f"{c.name}: h_hist differs"
            assert torch.equal(c_s[int(zero_c0):], c_g[int(zero_c0):]), f"{c.name}: c_hist differs"
            assert torch.equal(g_s, g_g), f"{c.name}: gates differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_group_step_equals_a_group_forward_of_one_step(dtype):
    """convlstm_group_step with carried state into NaN-filled buffers against convlstm_group_forward on x_t[None], h0, c0: the new
    state is slot 1 of the histories, bit for bit."""
    ops.GROUP_LSTM, ops.HOIST_X = True, False
    cases = [RCase(**{**c.__dict__, "T": 1, "state": True}) for c in GROUP]
    ds = [{k: (None if v is None else v.to(DEV)) for k, v in RC.make_inputs(c, dtype).items()} for c in cases]
    outs = [(torch.full_like(d["h0"], float("nan")), torch.full_like(d["c0"], float("nan"))) for d in ds]
    with torch.no_grad():
        assert ops.convlstm_group_step([(d["x_all"][0], d["h0"], d["c0"], h_out, c_out, d["weight"], d["bias"], c.Hd, c.Cx)
                                        for c, d, (h_out, c_out) in zip(cases, ds, outs)]) is True
        res = ops.convlstm_group_forward([(d["x_all"][0][None], d["h0"], d["c0"], d["weight"], d["bias"], c.Hd, c.Cx) for c, d in zip(cases, ds)],
                                         False)
        torch.cuda.synchronize()
    for c, (h_out, c_out), (h_hist, c_hist, gates) in zip(cases, outs, res):
        assert gates is None
        assert torch.equal(h_out, h_hist[1]), f"{c.name}: h_out differs from h_hist[1]"
        assert torch.equal(c_out, c_hist[1]), f"{c.name}: c_out differs from c_hist[1]"


# ---------------------------------------------------------------------------------------------
# 5. inference forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
@pytest.mark.parametrize("name", ["A-state", "S-state"])
def test_inference_forms_equal_the_training_forward(name, dtype):
    c = RC.BY_NAME[name]
    inp = RC.make_inputs(c, dtype)
    d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
    x, h0, c0, w, b = d["x_all"], d["h0"], d["c0"], d["weight"], d["bias"]
    ops.HOIST_X = False
    h0_before = h0.clone()
    with torch.no_grad():
        h_tr, c_tr = ops.ConvLSTMSeq.apply(x, h0, c0, w, b, c.Hd, c.Cx, True)
        h_in, c_in = ops.ConvLSTMSeq.apply(x, h0, c0, w, b, c.Hd, c.Cx, False)                 # the direct form: step 0 reads h0 / c0 in place
        assert torch.equal(h_in, h_tr) and torch.equal(c_in, c_tr) and torch.equal(h0, h0_before)
        h1_tr, c1_tr = ops.ConvLSTMSeq.apply(x[:1], h0, c0, w, b, c.Hd, c.Cx, True)
        h1_tr, c1_tr = h1_tr.clone(), c1_tr.clone()
        h_out, c_out = torch.full_like(h0, float("nan")), torch.full_like(c0, float("nan"))
        r_h, r_c = ops.ConvLSTMSeq.apply(x[:1], h0, c0, w, b, c.Hd, c.Cx, False, (h_out, c_out))
        assert r_h.data_ptr() == h_out.data_ptr() and r_c.data_ptr() == c_out.data_ptr()
        assert torch.equal(h_out, h1_tr[0]) and torch.equal(c_out, c1_tr) and torch.equal(h0, h0_before)
        c_io = c0.clone()                                                                       # c_out is c0 itself
        h_out2 = torch.full_like(h0, float("nan"))
        ops.ConvLSTMSeq.apply(x[:1], h0, c_io, w, b, c.Hd, c.Cx, False, (h_out2, c_io))
        assert torch.equal(h_out2, h1_tr[0]) and torch.equal(c_io, c1_tr)
        # the documented refusals
        with pytest.raises(L.UclstmError):
            ops.ConvLSTMSeq.apply(x[:2], h0, c0, w, b, c.Hd, c.Cx, False, (h_out, c_out))
        with pytest.raises(L.UclstmError):
            ops.ConvLSTMSeq.apply(x[:1], h0, c0, w, b, c.Hd, c.Cx, True, (h_out, c_out))
        with pytest.raises(L.UclstmError):
            ops.ConvLSTMSeq.apply(x[:1], h0, c0, w, b, c.Hd, c.Cx, False, (h0, c_out))
        with pytest.raises(L.UclstmError):
            ops.ConvLSTMSeq.apply(x[:1], h0, c0, w, b, c.Hd, c.Cx, False, (h_out.float(), c_out))
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 6. module level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_two_layer_module_equals_two_chained_sequences_and_each_checks_step_by_step(dtype):
    """ConvLSTM(24, 40, num_layers=2), a given state for layer 0 and None for layer 1: outputs, final states and every gradient
    are bit-identical to two ConvLSTMSeq.apply calls chained by hand, and both traced layers pass the step-by-step check (the
    dh_all that reaches layer 0 is captured with a hook on the intermediate)."""
    c0_ = RCase("M-layer0", 3, 2, 9, 10, 24, 40, state=True, dc_T=True)
    c1_ = RCase("M-layer1", 3, 2, 9, 10, 40, 40, dc_T=True)
    i0, i1 = RC.make_inputs(c0_, dtype), RC.make_inputs(c1_, dtype, seed=1)
    ops.HOIST_X, ops.ASYNC_WGRAD = False, False
    torch.manual_seed(0)
    m = U.ConvLSTM(24, 40, num_layers=2).to(DEV)
    with torch.no_grad():
        for layer, i in zip(m.layers, (i0, i1)):
            layer.conv.weight.copy_(i["weight"])
            layer.conv.bias.copy_(i["bias"])
    params = [p for layer in m.layers for p in (layer.conv.weight, layer.conv.bias)]

    def leaves():
        x = i0["x_all"].to(DEV).requires_grad_()
        return x, i0["h0"].to(DEV).requires_grad_(), i0["c0"].to(DEV).requires_grad_()

    gouts = [i1["dh_all"].to(DEV), i0["dc_T"].to(DEV), i1["dc_T"].to(DEV)]
    x, h0, c0 = leaves()
    with ops.compute_dtype(dtype):
        out, states = m.seq_nhwc(x, [(h0, c0), None])
    got = torch.autograd.grad([out, states[0][1], states[1][1]], [x, h0, c0] + params, gouts)
    # by hand, traced
    x, h0, c0 = leaves()
    ops.RECURRENCE_TRACE, ops.LAUNCH_LOG = trace, llog = [], []
    a, ca = ops.ConvLSTMSeq.apply(x, h0, c0, params[0], params[1], 40, 24, True)
    captured = []
    a.register_hook(lambda g: captured.append(g.detach().clone()))
    bb, cb = ops.ConvLSTMSeq.apply(a, None, None, params[2], params[3], 40, 40, True)
    want = torch.autograd.grad([bb, ca, cb], [x, h0, c0] + params, gouts)
    torch.cuda.synchronize()
    assert torch.equal(out, bb) and torch.equal(states[0][1], ca) and torch.equal(states[1][1], cb)
    assert torch.equal(states[0][0], a[-1]) and torch.equal(states[1][0], bb[-1])
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_)
    assert [e[0] for e in trace] == ["fwd", "fwd", "bwd", "bwd"] and len(captured) == 1
    splits = [int(e[4]) for e in llog if e[0] == "wgrad"]
    cpu = lambda t: t.detach().cpu()
    i1 = dict(i1, x_all=cpu(a))
    i0 = dict(i0, dh_all=cpu(captured[0]))
    for c, inp, f, bw, outs, sp in ((c1_, i1, trace[1], trace[2], dict(dx=captured[0], dW=want[5], db=want[6]), splits[0]),
                                    (c0_, i0, trace[0], trace[3], dict(dx=want[0], dh0=want[1], dc0=want[2], dW=want[3], db=want[4]), splits[1])):
        run = dict(inp=inp, x_all=inp["x_all"], h_hist=cpu(f[1]), c_hist=cpu(f[2]), gates=cpu(f[3]), dgates=cpu(bw[1]),
                   out={k: cpu(v) for k, v in outs.items()}, splits=sp)
        # (the dh_all that reaches layer 0 is a computed gradient: only the chosen gradients are held to the fp16 magnitudes)
        check_run(c, dtype, RC.plan_of(c), run, name="module " + c.name, chosen=("dc_T",) if c is c0_ else ("dh_all", "dc_T"))
