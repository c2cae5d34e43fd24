"""ops.convlstm_tick: one inference step of n independent ConvLSTM layers with carried state, whatever their sizes.

The members are the five recurrences of PretrainedTemporalUNet at 64 x 64 and B = 1 -- 1024, 256, 64, 16 and 4 pixels per step --
with reduced widths (64, 64, 128, 128, 256) so that the f64 references take seconds.  What is checked:

  * a member whose step the library runs on the 128 x 128 per-tap shape is bit-identical to the same step through ConvLSTMSeq alone
    (the tap group launch keeps each member's own K split);
  * a patch-shape member that shares its launch takes its K ranges from plan_group_ksplit, so it is compared with the f64 cell of
    tests/recurrence_cases.py on the device's own stored inputs, inside that file's forward bounds for the plan that ran;
  * the launches recorded in ops.LAUNCH_LOG are the partition that uclstm_igemm_fwd_shape implies for the members' step
    descriptors (computed here from the library's planners, not written down);
  * GROUP_LSTM = False launches every member alone, with the same bits;
  * a member without state or with h_out aliasing h_prev raises.
"""
import ctypes as C

import pytest
import torch

import igemm_cases as IC
import recurrence_cases as RC
from recurrence_cases import RCase
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
SWITCHES = ("GROUP_LSTM", "LAUNCH_LOG", "HOIST_X")

# (pixels, width) of the model's five recurrences at 64 x 64, B = 1, widths reduced: lstm_skips[1], [2], [3], [4], lstm
MODEL = [RCase("K-1024", 1, 1, 32, 32, 64, 64, state=True), RCase("K-256", 1, 1, 16, 16, 64, 64, state=True),
         RCase("K-64", 1, 1, 8, 8, 128, 128, state=True), RCase("K-16", 1, 1, 4, 4, 128, 128, state=True),
         RCase("K-4", 1, 1, 2, 2, 256, 256, state=True)]
# five members of the per-tap shape: more than one launch holds; one with padded channels, one that splits onto the 64 x 256 shape
MANY = [RCase("M-a", 1, 1, 4, 4, 128, 128, state=True), RCase("M-b", 1, 2, 3, 5, 24, 40, state=True),
        RCase("M-c", 1, 1, 2, 2, 64, 64, state=True), RCase("M-d", 1, 1, 8, 8, 64, 128, state=True),
        RCase("M-e", 1, 3, 9, 11, 24, 21, state=True), RCase("M-narrow", 1, 1, 8, 8, 64, 16, state=True)]


@pytest.fixture(autouse=True)
def restore_switches():
    saved = {k: getattr(ops, k) for k in SWITCHES}
    try:
        ops.HOIST_X = False
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def solo_plan(c):
    """(K ranges the member's step has alone, kind of launch the library's planners imply for that step)."""
    pd = ops.lstm_pack_desc(c.Hd, c.Cx, c.k)
    ks = ops.split_k_factor(c.pixels, pd.N, pd.Ktot // 64)
    ic = IC.Case(c.name, -1, c.B, c.H, c.W, [(c.Cxp, c.H, c.W, 0, 0), (c.Hdp, c.H, c.W, 0, 0)], pd.N, ktap=c.k, pad=c.k // 2,
                 epi=L.EPI_ATOMIC if ks > 1 else L.EPI_LSTM, ksplit=ks, Hd=c.Hd, bias=False)
    shape = int(L.lib.uclstm_igemm_fwd_shape(C.byref(IC.dummy_desc(ic))))
    return ks, "patch" if shape == 2 else "tap" if (shape == 0 and c.k == 3) else "single"


def expected(cases):
    """(LAUNCH_LOG "tick" entries, K ranges per member) of convlstm_tick over ``cases`` with GROUP_LSTM on."""
    solo = [solo_plan(c) for c in cases]
    ks = [s[0] for s in solo]
    log, split_members = [], 0
    for kind in ("patch", "tap"):
        idx = [i for i, s in enumerate(solo) if s[1] == kind]
        for j in range(0, len(idx), 4):
            chunk = idx[j:j + 4]
            if kind == "patch" and len(chunk) > 1:
                planned = ops.plan_group_ksplit([(((ops.lstm_pack_desc(cases[i].Hd, cases[i].Cx, 3).N + 127) // 128) * (cases[i].pixels // 256),
                                                  ops.lstm_pack_desc(cases[i].Hd, cases[i].Cx, 3).Ktot // (64 * 9)) for i in chunk])
                for i, k in zip(chunk, planned):
                    ks[i] = k
            log.append(("tick", kind, len(chunk)))
            split_members += sum(ks[i] > 1 for i in chunk)
    log += [("tick", "pointwise", min(4, split_members - j)) for j in range(0, split_members, 4)]
    log += [("tick", "single", 1) for s in solo if s[1] == "single"]
    return log, ks, [s[1] for s in solo]


def inputs(cases, dtype):
    return [RC.make_inputs(c, dtype) for c in cases]


def members(cases, inps, alias=None, no_c=None):
    ms, outs = [], []
    for i, (c, inp) in enumerate(zip(cases, inps)):
        d = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
        h_out, c_out = torch.full_like(d["h0"], float("nan")), torch.full_like(d["c0"], float("nan"))
        ms.append((d["x_all"][0], d["h0"], None if no_c == i else d["c0"], d["h0"] if alias == i else h_out, c_out, d["weight"], d["bias"],
                   c.Hd, c.Cx))
        outs.append((h_out, c_out))
    return ms, outs


def alone(cases, inps):
    """Every member stepped alone through ConvLSTMSeq with out=: the (h, c) a tick must reproduce."""
    ms, outs = members(cases, inps)
    with torch.no_grad():
        for (x_t, h0, c0, h_out, c_out, w, b, Hd, Cx) in ms:
            ops.ConvLSTMSeq.apply(x_t.unsqueeze(0), h0, c0, w, b, Hd, Cx, False, (h_out, c_out))
    torch.cuda.synchronize()
    return outs


def tick(cases, inps):
    ms, outs = members(cases, inps)
    ops.LAUNCH_LOG = log = []
    with torch.no_grad():
        ops.convlstm_tick(ms)
    torch.cuda.synchronize()
    ops.LAUNCH_LOG = None
    return outs, [e for e in log if e[0] == "tick"]


def same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
@pytest.mark.parametrize("cases", [MODEL, MANY], ids=["model", "many"])
def test_tick_partition_bits_and_f64(cases, dtype):
    ops.GROUP_LSTM = True
    inps = inputs(cases, dtype)
    want_log, ks, kinds = expected(cases)
    if cases is MODEL:          # the shapes this test is about: two patch members sharing a launch, three per-tap members sharing one
        assert kinds == ["patch", "patch", "tap", "tap", "tap"], kinds
    else:
        assert kinds.count("tap") == 5 and kinds.count("single") == 1, kinds
    ref = alone(cases, inps)
    got, log = tick(cases, inps)
    assert log == want_log, f"launches {log}, the members' step descriptors imply {want_log}"
    for c, inp, kind, k, (h, cc), (hr, cr) in zip(cases, inps, kinds, ks, got, ref):
        assert not bool(torch.isnan(h.float()).any()) and not bool(torch.isnan(cc).any()), f"{c.name}: state not written"
        if kind != "patch":
            assert same_bits(h, hr) and same_bits(cc, cr), f"{c.name} ({kind}): differs from the member stepped alone"
            continue
        r = RC.Ref(inp["weight"].to(dtype).double(), inp["bias"].double(), c.Hd, c.Cx, 3)
        pd = ops.lstm_pack_desc(c.Hd, c.Cx, 3)
        worst = RC.check_forward(c, dtype, r, [RC.f32_coeff(pd.Ktot, k)], inp["x_all"], torch.stack((inp["h0"], h.cpu())),
                                 torch.stack((inp["c0"], cc.cpu())), None, False)
        worst.pop("gates")
        print(f"[parity] tick {c.name} {RC.tag(dtype)} (patch, {k} K range(s)): worst |err| / bound " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
        assert all(v <= 1.0 for v in worst.values()), f"{c.name} {RC.tag(dtype)}: beyond the bound: {worst}"


@pytest.mark.parametrize("dtype", DTYPES, ids=RC.tag)
def test_group_switch_off_launches_every_member_alone_with_the_same_bits(dtype):
    inps = inputs(MODEL, dtype)
    ref = alone(MODEL, inps)
    ops.GROUP_LSTM = True
    on, _ = tick(MODEL, inps)
    ops.GROUP_LSTM = False
    off, log = tick(MODEL, inps)
    assert log == [("tick", "single", 1)] * len(MODEL), log
    kinds = expected(MODEL)[2]
    for c, kind, (h, cc), (hr, cr), (h1, c1) in zip(MODEL, kinds, off, ref, on):
        assert same_bits(h, hr) and same_bits(cc, cr), f"{c.name}: one by one differs from the member stepped alone"
        if kind == "tap":
            assert same_bits(h, h1) and same_bits(cc, c1), f"{c.name}: the group launch differs from the one-by-one path"


@pytest.mark.parametrize("mutate", ["alias", "no_c_prev"])
def test_tick_refuses_aliased_or_missing_state(mutate):
    ops.GROUP_LSTM = True
    inps = inputs(MODEL, torch.bfloat16)
    ms, outs = members(MODEL, inps, alias=3 if mutate == "alias" else None, no_c=1 if mutate == "no_c_prev" else None)
    with torch.no_grad(), pytest.raises(L.UclstmError):
        ops.convlstm_tick(ms)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(h.float()).all()) and bool(torch.isnan(c).all()) for h, c in outs), "a refused tick wrote a state"
