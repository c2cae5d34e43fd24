"""tests/recurrence_cases.py without a GPU:
  1. the step references, chained without any rounding, equal f64 autograd through F.conv2d (oracle.convlstm_cell) for every output;
  2. an f32 emulation of the device plan (F.conv2d in f32, 16-bit rounding where the kernels store, K-range slabs added in f32) lies
     inside every bound of the step-by-step comparison, on every case and in both 16-bit types;
  3. eight wrong recurrences (one wrong index or one dropped term each) fall outside a bound on a named case;
  4. the plan of every case -- K ranges, slabs and kernel of the per-step GEMM and of the W_h^T launch -- is the one it is meant for.
"""
import pytest
import torch
import torch.nn.functional as F

import recurrence_cases as RC
from oracle import unet_oracle as O
from unet_convlstm_amd import ops

F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16]


def nchw(t, Cv):
    """[..., H, W, Cp] -> [..., Cv, H, W]"""
    return t[..., :Cv].movedim(-1, -3).contiguous()


def nhwc(t, Cp):
    """[..., C, H, W] -> [..., H, W, Cp] with zero pad channels"""
    return RC.pad_last(t.movedim(-3, -1).contiguous(), Cp)


# ---------------------------------------------------------------------------------------------
# 1. reference against autograd
# ---------------------------------------------------------------------------------------------
def chained_reference(ref, x_all, h0, c0, dh_all, dc_T):
    """The step references of recurrence_cases chained in f64, nothing rounded: what check_forward / check_backward compare with,
    fed with its own outputs instead of the device's."""
    T, B, H, W, _ = x_all.shape
    Hdp, M = ref.Hdp, B * H * W
    sh = (B, H, W, Hdp)
    h = [torch.zeros(sh, dtype=F64) if h0 is None else h0]
    c = [torch.zeros(sh, dtype=F64) if c0 is None else c0]
    gates = []
    for t in range(T):
        g, cn, hn, _ = ref.fwd_step(x_all[t], h[t], None if (c0 is None and t == 0) else c[t])
        gates.append(g)
        h.append(hn.reshape(sh))
        c.append(cn.reshape(sh))
    dc = dc_T.reshape(M, Hdp)
    dg = [None] * T
    for t in range(T - 1, -1, -1):
        rec = ref.dgrad(dg[t + 1].reshape(B, H, W, 4 * Hdp), "h")[0] if t < T - 1 else 0.0
        dg[t], _, dc = RC.Ref.bwd_step(gates[t], c[t].reshape(M, Hdp), c[t + 1].reshape(M, Hdp), dh_all[t].reshape(M, Hdp) + rec, dc)
    dgs = torch.stack(dg).reshape(T, B, H, W, 4 * Hdp)
    return dict(h_all=torch.stack(h[1:]), c_T=c[T], dx=ref.dgrad(dgs.reshape(T * B, H, W, -1), "x")[0].reshape(T, B, H, W, -1),
                dh0=ref.dgrad(dgs[0], "h")[0].reshape(sh), dc0=dc.reshape(sh), dW=ref.wgrad(x_all, torch.stack(h[:T]), dgs)[0],
                db=ref.bgrad(dgs)[0])


@pytest.mark.parametrize("state", [False, True], ids=["zero-state", "given-state"])
@pytest.mark.parametrize("Hd,Cx,T,B,H,W", [(5, 3, 3, 2, 5, 6), (40, 12, 2, 1, 4, 5)], ids=["Hd5", "Hd40"])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_chained_step_references_equal_f64_autograd(k, Hd, Cx, T, B, H, W, state):
    torch.manual_seed(100 * k + Hd + int(state))
    Hdp, Cxp = ops.cpad(Hd), ops.cpad(Cx)
    w = (torch.randn(4 * Hd, Cx + Hd, k, k, dtype=F64) * 0.3).requires_grad_()
    b = (torch.randn(4 * Hd, dtype=F64) * 0.3).requires_grad_()
    x = torch.randn(T, B, Cx, H, W, dtype=F64, requires_grad=True)
    h0 = (torch.randn(B, Hd, H, W, dtype=F64) * 0.5).requires_grad_() if state else None
    c0 = torch.randn(B, Hd, H, W, dtype=F64, requires_grad=True) if state else None
    dh_all, dc_T = torch.randn(T, B, Hd, H, W, dtype=F64), torch.randn(B, Hd, H, W, dtype=F64)
    h, c, hs = h0, c0, []
    for t in range(T):
        h, c = O.convlstm_cell(x[t], h, c, w, b)
        hs.append(h)
    h_all = torch.stack(hs)
    ins = [x, w, b] + ([h0, c0] if state else [])
    grads = torch.autograd.grad([h_all, c], ins, [dh_all, dc_T])
    want = dict(h_all=nhwc(h_all.detach(), Hdp), c_T=nhwc(c.detach(), Hdp), dx=nhwc(grads[0], Cxp), dW=grads[1].reshape(-1), db=grads[2])
    if state:
        want.update(dh0=nhwc(grads[3], Hdp), dc0=nhwc(grads[4], Hdp))
    ref = RC.Ref(w.detach(), b.detach(), Hd, Cx, k)
    got = chained_reference(ref, nhwc(x.detach(), Cxp), None if h0 is None else nhwc(h0.detach(), Hdp),
                            None if c0 is None else nhwc(c0.detach(), Hdp), nhwc(dh_all, Hdp), nhwc(dc_T, Hdp))
    for key, wv in want.items():
        torch.testing.assert_close(got[key].reshape(wv.shape), wv, rtol=1e-12, atol=1e-13, msg=lambda m: f"{key}: {m}")


# ---------------------------------------------------------------------------------------------
# 2. / 3. f32 emulation of the device plan, right and wrong
# ---------------------------------------------------------------------------------------------
MUTANTS = {                      # name -> the case on which it must fall outside a bound
    "drop_dh_at_one_t": "A",
    "c_prev_from_next_slot": "A-state",
    "other_buffer": "A-T5",
    "missing_slab": "A",
    "ignore_dc_T": "A-no-dh",
    "wgrad_h_next": "A",
    "bias_first_columns": "P5",
    "dc_not_times_f": "A",
}


def emulate(c, dtype, inp, plan, mutant=None):
    """The device plan in f32 on the CPU.  Returns what a device run leaves: the stored histories and the outputs, NHWC, padded."""
    r = lambda t: t.to(dtype).float()
    T, B, H, W, Hd, Cx, k, Hdp, Cxp = c.T, c.B, c.H, c.W, c.Hd, c.Cx, c.k, c.Hdp, c.Cxp
    p = k // 2
    w, b = r(inp["weight"]), inp["bias"].float()
    x = nchw(inp["x_all"].float(), Cx)
    zero = torch.zeros(B, Hd, H, W)
    h = [zero if inp["h0"] is None else nchw(inp["h0"].float(), Hd)]
    cs = [zero if inp["c0"] is None else nchw(inp["c0"], Hd)]
    gates = []
    for t in range(T):
        if plan["hoist"]:
            pre = F.conv2d(x[t], w[:, :Cx], None, padding=p) + F.conv2d(h[t], w[:, Cx:], None, padding=p) + b[None, :, None, None]
        else:
            pre = F.conv2d(torch.cat((x[t], h[t]), 1), w, b, padding=p)
        pi, pf, pg, po = pre.view(B, 4, Hd, H, W).unbind(1)
        gi, gf, gg, go = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
        cn = gf * cs[t] + gi * gg
        cs.append(cn)
        h.append(r(go * torch.tanh(cn)))
        gates.append(r(torch.stack((gi, gf, gg, go), 1)))
    # backward: W_h^T over the padded dgates channels, K ranges of whole 64-channel chunks
    _, ks_b, nsl_b, _ = plan["dh"]
    chunks = ops.kseg(4 * Hdp) // 64
    cpr = -(-chunks // ks_b)
    wh_p = torch.zeros(4, Hdp, Hd, k, k)
    wh_p[:, :Hd] = w[:, Cx:].view(4, Hd, Hd, k, k)
    wh_p = wh_p.view(4 * Hdp, Hd, k, k)

    def dh_rec_of(dg):                   # dg [B,4,Hd,H,W] -> f32 sum of the slabs, or the 16-bit store
        if dg is None:
            return zero
        dgp = torch.zeros(B, 4, Hdp, H, W)
        dgp[:, :, :Hd] = dg
        dgp = dgp.view(B, 4 * Hdp, H, W)
        slabs = [F.conv_transpose2d(dgp[:, lo:lo + 64 * cpr], wh_p[lo:lo + 64 * cpr], padding=p) for lo in range(0, 4 * Hdp, 64 * cpr)]
        assert len(slabs) == nsl_b
        if mutant == "missing_slab":
            assert len(slabs) >= 2
            del slabs[1]
        tot = slabs[0]
        for s in slabs[1:]:
            tot = tot + s
        return r(tot) if ks_b == 1 else tot

    dh_all = None if inp["dh_all"] is None else nchw(inp["dh_all"].float(), Hd)
    dc = zero if (inp["dc_T"] is None or mutant == "ignore_dc_T") else nchw(inp["dc_T"], Hd)
    dg = [None] * (T + 2)
    for t in range(T - 1, -1, -1):
        gi, gf, gg, go = gates[t].unbind(1)
        cp = cs[t + 1] if mutant == "c_prev_from_next_slot" else cs[t]
        dh = zero if (dh_all is None or (mutant == "drop_dh_at_one_t" and t == 1)) else dh_all[t]
        dh = dh + dh_rec_of(dg[t + 2] if mutant == "other_buffer" else dg[t + 1])
        tc = torch.tanh(cs[t + 1])
        dct = dc + dh * go * (1 - tc * tc)
        dg[t] = r(torch.stack((dct * gg * gi * (1 - gi), dct * cp * gf * (1 - gf), dct * gi * (1 - gg * gg), dh * tc * go * (1 - go)), 1))
        dc = dct if mutant == "dc_not_times_f" else dct * gf
    dgs = torch.stack(dg[:T])                                   # [T,B,4,Hd,H,W]
    flat = dgs.view(T * B, 4 * Hd, H, W)
    hprev = torch.stack(h[1:] if mutant == "wgrad_h_next" else h[:T])
    dW = torch.nn.grad.conv2d_weight(torch.cat((x, hprev), 2).view(T * B, Cx + Hd, H, W), w.shape, flat, padding=p)
    dgs_p = torch.zeros(T, B, 4, Hdp, H, W)
    dgs_p[:, :, :, :Hd] = dgs
    dg_nhwc = dgs_p.view(T, B, 4 * Hdp, H, W).movedim(-3, -1).contiguous()
    db = dg_nhwc.reshape(-1, 4 * Hdp).sum(0)
    db = db[:4 * Hd] if mutant == "bias_first_columns" else db.view(4, Hdp)[:, :Hd].reshape(-1)
    g_nhwc = nhwc(torch.stack(gates), Hdp).permute(0, 1, 3, 4, 2, 5).contiguous()        # [T,B,H,W,4,Hdp]
    g_nhwc[..., Hd:] = torch.tensor([0.5, 0.5, 0.0, 0.5])[:, None]      # pad hidden channels are computed from zero panel rows
    return dict(x_all=inp["x_all"], h_hist=nhwc(torch.stack(h), Hdp).to(dtype), c_hist=nhwc(torch.stack(cs), Hdp),
                gates=g_nhwc.to(dtype), dgates=dg_nhwc.to(dtype),
                out=dict(dx=nhwc(r(F.conv_transpose2d(flat, w[:, :Cx], padding=p)).view(T, B, Cx, H, W), Cxp), dW=dW, db=db,
                         dh0=nhwc(r(dh_rec_of(dg[0])), Hdp) if c.state else None, dc0=nhwc(dc, Hdp) if c.state else None))


def compare(c, dtype, inp, plan, run):
    ref = RC.Ref(inp["weight"].to(dtype).double(), inp["bias"].double(), c.Hd, c.Cx, c.k)
    zero_c0 = inp["c0"] is None
    worst = RC.check_forward(c, dtype, ref, RC.fwd_coeffs(c, plan, zero_c0), run["x_all"], run["h_hist"], run["c_hist"], run["gates"], zero_c0)
    worst.update(RC.check_backward(c, dtype, ref, plan, x_all=run["x_all"], h_hist=run["h_hist"], c_hist=run["c_hist"], gates=run["gates"],
                                   dgates=run["dgates"], dh_all=inp["dh_all"], dc_T=inp["dc_T"], has_c0=not zero_c0, out=run["out"]))
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_f32_emulation_lies_inside_every_bound(name, dtype):
    c = RC.BY_NAME[name]
    inp, plan = RC.make_inputs(c, dtype), RC.plan_of(c)
    worst = compare(c, dtype, inp, plan, emulate(c, dtype, inp, plan))
    print(f"[parity] emulation {name} {RC.tag(dtype)}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), f"{name}: a correct f32 recurrence leaves the bounds: {worst}"
    assert {"c", "h", "gates", "dgates", "dx", "dW", "db"} <= set(worst) and (("dh0" in worst and "dc0" in worst) or not c.state)


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_wrong_recurrences_fall_outside_the_bounds(mutant, dtype):
    c = RC.BY_NAME[MUTANTS[mutant]]
    inp, plan = RC.make_inputs(c, dtype), RC.plan_of(c)
    worst = compare(c, dtype, inp, plan, emulate(c, dtype, inp, plan, mutant))
    print(f"[parity] mutant {mutant} on {c.name} {RC.tag(dtype)}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) > 1.0, f"{mutant} on {c.name}: a wrong recurrence stays inside every bound: {worst}"


# ---------------------------------------------------------------------------------------------
# 4. plans
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_case_reaches_the_plan_it_is_meant_for(name):
    c = RC.BY_NAME[name]
    p = RC.plan_of(c)
    assert (p["fwd"][1:], p["dh"][1:]) == c.plan, f"{name}: plan {p}"
    assert p["hoist"] == (c.hoist and c.T >= 2)
    if name in ("A", "A-state"):        # the plans the issue names: two K ranges in slabs forward, 27 K-steps in three slabs backward
        assert p["fwd"][0] // 64 == 18 and p["dh"][0] // 64 == 27
    if name == "S":
        assert p["dh"][0] // 64 == 9
    if name == "A-k1":
        assert p["fwd"][0] // 64 == 2
