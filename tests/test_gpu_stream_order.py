"""Cross-stream hand-offs under injected delays, bit for bit.

Every hand-off of tests/stream_order_cases.py's inventory is correct only if somebody wrote a wait, an event or a ``record_stream``,
and at natural timing a missing one still gives the right bits: the host enqueues so slowly that the side stream is never behind.
Here the schedule is bent with ``uclstm_stream_spin``: the spin in front of every hand-off on the delayed stream is sized from the
measured device time of the undelayed step so that the stream falls behind by at least twice that time (stream_order_cases.plan_spin),
and the result must be ``torch.equal`` to the ``one_stream`` run, in which the side stream IS the main stream and nothing can race.
Everything runs under ``ops.deterministic()``, where two runs from identical state agree bit for bit
(tests/test_gpu_deterministic.py::test_two_deterministic_steps_from_identical_state_are_bit_identical): there is no tolerance.

A   one operator, forward + backward with attached f32 ``.grad`` buffers: ``one_stream`` against ``slow_side``;
A'  the same with reallocation pressure: references dropped and NaN tensors of the same sizes allocated on the main stream before
    any synchronisation (after the forward pass and after ``backward()`` has returned on the host);
B   three consecutive ``train_step``s under ``one_stream`` / ``slow_side`` / ``slow_main`` / ``both``, no synchronisation between the steps;
C   a step captured under ``slow_side`` (the spins are nodes of the side branch) against eager ``one_stream`` steps (child process);
D   ``FlatDDP`` on one rank over RCCL, f32 buckets and bf16 staging;
E   the control, once: without the join the delayed gradient IS seen missing -- the schedule has power.

Every case runs once per schedule; nothing here repeats a run until it differs.  Figures are printed (run with -s).
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import train_loop_cases as TL
import resnet_cases as RC
import stream_order_cases as SO

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import modules as M
    from unet_convlstm_amd import ops
    from unet_convlstm_amd import resnet as R
    from test_gpu_deterministic import LARGE, first_difference

DEV = "cuda"
F32 = torch.float32


@pytest.fixture(autouse=True)
def restore_switches():
    saved = (ops.PREPACK, ops.PACK_BATCHED, ops.is_deterministic(), ops.get_compute_dtype())
    ops.prepack_end()
    ops._PACK_PLAN.clear()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        ops.PREPACK, ops.PACK_BATCHED = saved[:2]
        ops.set_deterministic(saved[2])
        ops.set_compute_dtype(saved[3])
        ops.prepack_end()
        ops._PACK_PLAN.clear()


@pytest.fixture(scope="module", autouse=True)
def release_references():
    yield
    _OP_REF.clear()
    _OP_LOG.clear()
    torch.cuda.empty_cache()


def device():
    return torch.device(DEV, torch.cuda.current_device())


PROBE_US = 2000          # ops._streams_overlap reports "serialised" when the second spin ends later than 1.5 x this after the first
                         # began: two spins on one queue take 2 x, and a pause of the host between the two launches (the collector
                         # after a model was built) counts against the 0.5 x of slack -- 1 ms here, where the default 300 us leaves 150 us


def overlap(a, b):
    return ops._streams_overlap(a, b, spin_us=PROBE_US)


def require_overlap():
    """Where side and main share a hardware queue a spin on the side stream delays nothing: the test must fail, not pass."""
    main = torch.cuda.current_stream()
    side = ops.side_stream(device())
    assert side != main and overlap(main, side), \
        "the side stream does not run concurrently with the main stream on this machine: a spin on it delays nothing, so a delayed " \
        "schedule would prove nothing"


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same(a, b):
    """Bit-identical, compared on the device."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def compare(what, ref, got, names=(), sizes=()):
    """Every tensor of ``got`` equals ``ref``'s bit for bit; the message names the first differing tensor (first_difference of
    tests/test_gpu_deterministic.py, the flat buffers resolved to parameter names)."""
    assert list(ref) == list(got), f"{what}: different tensors {sorted(set(ref) ^ set(got))}"
    if all(same(ref[k], got[k]) for k in ref):
        return
    bad = [k for k in ref if not same(ref[k], got[k])]
    nans = [k for k in bad if got[k].is_floating_point() and bool(torch.isnan(got[k]).any())]
    diff = first_difference({k: ref[k].cpu() for k in bad}, {k: got[k].cpu() for k in bad}, list(names), list(sizes))
    raise AssertionError(f"{what}: {len(bad)} of {len(ref)} tensors differ from the one_stream run; first: {diff}; holding NaN: {nans[:4]}")


def report(what, step_us, handoffs, spin, injected_us, stream="side"):
    print(f"[stream order] {what}: undelayed {step_us:.0f} us, {handoffs} {stream} hand-offs, spin {spin.reps} x {spin.us} us each, "
          f"injected {injected_us} us on the {stream} stream ({injected_us / max(step_us, 1e-9):.1f} x)")
    assert spin.us <= SO.MAX_SPIN_US
    assert injected_us >= SO.MIN_TOTAL_FACTOR * step_us, f"{what}: {injected_us} us injected for an undelayed time of {step_us:.0f} us"


# ---------------------------------------------------------------------------------------------
# A, A', E. operators
# ---------------------------------------------------------------------------------------------
def nhwc(x):
    """f32 NCHW -> 16-bit NHWC leaf that wants a gradient (so the input-gradient GEMMs run beside the weight gradients)."""
    with torch.no_grad():
        a = ops.ToNHWC.apply(x.to(DEV))
    return a.requires_grad_(True)


def joined(outs):
    """What a public forward does before it hands its result out (the operators below that call forward_nhwc themselves)."""
    ops.join_forward_side(device())
    return outs


def leaf(*shape):
    return (torch.randn(*shape) * 0.8).to(DEV).requires_grad_(True)


def op_doubleconv(B=2, H=16, W=16):
    m = M.DoubleConv(8, 12)
    return [m], [leaf(B, 8, H, W)], lambda xs: [m(xs[0])]


def op_down():
    m = M.Down(8, 16)
    return [m], [leaf(2, 8, 16, 16)], lambda xs: [m(xs[0])]


def op_up_two_sources():
    m = M.Up(16, 8)          # ConvT2x2 16 -> 8, then conv over cat([skip 8, up 8]); the skip is larger: centred at (1, 1)
    return [m], [leaf(2, 16, 7, 7), leaf(2, 8, 16, 16)], lambda xs: [m(xs[0], xs[1])]


def op_stage_pool_groups(B=2, T=3):
    m = M.DoubleConv(8, 24)          # T BatchNorm groups, the pooling fused into the second stage: (activation, pooled)
    return [m], [nhwc(torch.randn(T * B, 8, 16, 16))], lambda xs: joined(list(m.forward_nhwc(xs[0], groups=T, pool=True)))


def op_stage_64ch_16x64():
    m = M.DoubleConv(64, 64)         # the ring weight-gradient kernel and the slab unpack
    return [m], [nhwc(torch.randn(2, 64, 16, 64))], lambda xs: joined([m.forward_nhwc(xs[0])])


def op_encode_once():
    m = M.TemporalUNetDualView(1, 1, base_ch=8)          # the encoder of the model: im2col first layer, pooling fused into four stages

    def forward(xs):
        xb, skips = m.encode_once(xs[0])
        return [xb] + list(skips)
    return [m], [torch.randn(2, 2, 16, 16).to(DEV)], forward


def op_convt():
    m = torch.nn.ConvTranspose2d(16, 8, 2, stride=2)
    return [m], [nhwc(torch.randn(6, 16, 8, 8))], lambda xs: [ops.ConvT2x2.apply(xs[0], m.weight, m.bias)]


def op_convlstm(B=2, T=3):
    m = M.ConvLSTM(8, 16, num_layers=2)

    def forward(xs):
        seq, states = m([xs[0][:, t] for t in range(T)])
        return list(seq) + [states[-1][1]]
    return [m], [leaf(B, T, 8, 16, 16)], forward


def op_lstm_group(B=2, T=3):
    """Two independent 64-channel recurrences through convlstm_group_forward, each with its own ConvLSTMSeqPre node."""
    cells = [M.ConvLSTMCell(64, 64), M.ConvLSTMCell(64, 64)]
    sizes = [(16, 8), (16, 16)]

    def forward(xs):
        full = [(x.view(T, B, *x.shape[1:]), None, None, c.conv.weight, c.conv.bias, c.hidden_dim, c.input_dim) for x, c in zip(xs, cells)]
        assert ops.convlstm_group_ok(full), "the grouped recurrence does not take these shapes"
        pre = ops.convlstm_group_forward(full, True)
        outs = [ops.ConvLSTMSeqPre.apply(*f, True, hh, ch, gt) for f, (hh, ch, gt) in zip(full, pre)]
        return [o[0] for o in outs] + [o[1] for o in outs]
    return cells, [nhwc(torch.randn(T * B, 64, h, w) * 0.5) for h, w in sizes], forward


def op_resnet_block():
    """The trainable encoder's route: EncConv (stride 2 with the downsample conv1x1) + BnRelu + EncConv + BnAddRelu, training mode."""
    blk = R.BasicBlock(64, 128, 2)          # layer2's first block
    return [blk], [nhwc(torch.randn(4, 64, 16, 16))], \
        lambda xs: joined([R.PretrainedTemporalUNet._block(R.PretrainedTemporalUNet, xs[0], blk, [], True)])


def op_train_then_eval():
    """The joins in front of evaluation-mode BatchNorm: a training-mode forward_nhwc leaves its running-statistics updates on the side
    stream and nobody joins; the evaluation-mode pass right behind it reads those statistics -- with a backward pass through
    ops.conv_bn_stats, under no_grad through ops.conv_bn_fold."""
    m = M.DoubleConv(8, 12)

    def forward(xs):
        try:
            a1 = m.forward_nhwc(xs[0])
            m.eval()
            e_grad = m.forward_nhwc(xs[0])
            m.train()
            a2 = m.forward_nhwc(xs[0])
            m.eval()
            with torch.no_grad():
                e_fold = m.forward_nhwc(xs[0])
        finally:
            m.train()
        return [a1, e_grad, a2], {"evaluation output (with backward)": e_grad.detach().clone(), "evaluation output (fold)": e_fold}
    return [m], [nhwc(torch.randn(2, 8, 16, 16))], forward


def op_unet_forward():
    m = M.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True)          # the public forward of the model, training mode
    return [m], [torch.randn(2, 3, 2, 32, 32).to(DEV)], lambda xs: list(m(xs[0])[0])


def op_unet_step_nhwc():
    m = M.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True)          # one frame, training mode: the join before the output conv
    return [m], [torch.randn(2, 2, 32, 32).to(DEV)], lambda xs: [m.step_nhwc(xs[0])[0]]


def op_resnet_forward():
    m, (x, _, _) = build_resnet()          # the public forward of PretrainedTemporalUNet, every encoder stage trainable
    return [m], [x], lambda xs: [m(xs[0])[0]]


OPERATORS = {
    "doubleconv": op_doubleconv, "down": op_down, "up-two-sources": op_up_two_sources, "stage-pool-groups": op_stage_pool_groups,
    "stage-64ch-16x64": op_stage_64ch_16x64, "encode-once": op_encode_once, "convt": op_convt, "convlstm": op_convlstm,
    "lstm-group": op_lstm_group, "resnet-block": op_resnet_block, "train-then-eval": op_train_then_eval, "unet-forward": op_unet_forward,
    "unet-step-nhwc": op_unet_step_nhwc, "resnet-forward": op_resnet_forward,
}
_OP_REF = {}          # case -> (one_stream result, step time in us, side hand-offs), shared by A, A' and E
_OP_LOG = {}          # case -> ops.LAUNCH_LOG of that run


def pressure(shapes, rounds=2):
    """NaN tensors of the same sizes and dtypes on the main stream (plus a few small f32 ones, the sizes of BatchNorm sums and
    statistics), ``rounds`` times over: whatever the allocator hands back is overwritten."""
    small = [(n,) for n in (16, 48, 64, 128, 256, 1024, 4096) for _ in range(3)]
    for _ in range(rounds):
        held = [torch.full(shape, float("nan"), dtype=dtype, device=DEV) for shape, dtype in shapes]
        held += [torch.full(shape, float("nan"), dtype=F32, device=DEV) for shape in small]
        del held


def run_operator(case, realloc=False, after_backward=None):
    """Forward + backward of one operator from seed 11 with attached contiguous f32 gradient buffers (start value P != 0).
    The buffers are cloned on the main stream as soon as forward returns -- before backward, whose join would hide a missing
    join_forward_side, and before any synchronisation -- and again at the end.
    -> ({gradients, buffers after forward, buffers, input gradients}, device time of the pass in us)."""
    torch.manual_seed(11)
    mods, xs, forward = OPERATORS[case]()
    for m in mods:
        m.to(DEV).train()
    params = [(f"{i}.{k}", p) for i, m in enumerate(mods) for k, p in m.named_parameters() if p.requires_grad]
    for _, p in params:
        p.grad = (torch.randn(p.shape) * 0.05).to(DEV).contiguous()
    start = {name: p.grad.clone() for name, p in params} if after_backward is not None else None
    gen = torch.Generator().manual_seed(12)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    outs = forward(xs)
    outs, fwd_extra = outs if isinstance(outs, tuple) else (outs, {})
    fwd_buffers = {f"after forward: buffer {i}.{k}": b.detach().clone() for i, m in enumerate(mods) for k, b in m.named_buffers()}
    shapes = [(tuple(t.shape), t.dtype) for t in xs + outs]
    if realloc:
        pressure(shapes, 1)          # the forward pass's side work (running statistics) reads buffers the main stream has dropped
    gos = [(torch.randn(o.shape, generator=gen) * 0.5).to(DEV).to(o.dtype) for o in outs]
    torch.autograd.backward(outs, gos)
    e1.record()
    extra = after_backward(params, start) if after_backward is not None else {}
    dx = {f"dx{i}": x.grad for i, x in enumerate(xs) if x.grad is not None}
    if realloc:
        shapes += [(tuple(g.shape), g.dtype) for g in gos]
        del xs[:], outs[:], gos[:]
        pressure(shapes, 2)
    torch.cuda.synchronize()
    out = {name: p.grad.detach().clone() for name, p in params}
    out.update({f"buffer {i}.{k}": b.detach().clone() for i, m in enumerate(mods) for k, b in m.named_buffers()})
    out.update(fwd_buffers)
    out.update(fwd_extra)
    out.update(dx)
    out.update(extra)
    return out, e0.elapsed_time(e1) * 1e3


def operator_reference(case):
    """The one_stream run (twice: the first loads code objects and warms the allocator, and the two must agree -- the yardstick),
    its device time and the number of side hand-offs it made."""
    if case not in _OP_REF:
        with ops.deterministic(), SO.one_stream(ops, device()):
            first, _ = run_operator(case)
            ops.LAUNCH_LOG = []
            try:
                with SO.slow_side(ops, L) as count:
                    ref, us = run_operator(case)
                _OP_LOG[case] = list(ops.LAUNCH_LOG)
            finally:
                ops.LAUNCH_LOG = None
        compare(f"{case}: two one_stream runs", first, ref)
        assert count.handoffs >= 1, f"{case}: no side-stream hand-off happened, the side route was not taken"
        assert all(bool(torch.isfinite(v).all()) for v in ref.values() if v.is_floating_point())
        _OP_REF[case] = (ref, us, count.handoffs)
    return _OP_REF[case]


@pytest.mark.parametrize("case", list(OPERATORS))
def test_operator_gradients_under_a_delayed_side_stream(case):
    ref, us, n = operator_reference(case)
    require_overlap()
    spin = SO.plan_spin(us, n)
    with ops.deterministic(), SO.slow_side(ops, L, spin) as sched:
        got, _ = run_operator(case)
    report(f"A {case}", us, n, spin, sched.injected_us)
    assert sched.handoffs == n
    if case == "stage-64ch-16x64":          # ("wgrad", kernel shape, N, Ktot, slabs): the ring kernel (4), several slabs for the unpack to add
        ring = [e for e in _OP_LOG[case] if e[0] == "wgrad" and e[1] == 4 and e[4] > 1]
        assert len(ring) == 2, "the 64-channel case did not take the ring weight-gradient kernel with slabs: " \
                               f"{[e for e in _OP_LOG[case] if e[0] == 'wgrad']}"
    compare(f"A {case} under slow_side", ref, got)


@pytest.mark.parametrize("case", list(OPERATORS))
def test_operator_gradients_under_a_delayed_side_stream_and_reallocation(case):
    """The main stream is held back by the join at the end of backward(), so the NaN fills after it land behind the side stream's
    reads whatever the allocator hands out; the buffers this can catch are those the main stream drops and reuses BEFORE a join:
    the forward pass's statistics, and gradients freed while the backward pass is still running."""
    ref, us, n = operator_reference(case)
    require_overlap()
    spin = SO.plan_spin(us, n)
    with ops.deterministic(), SO.slow_side(ops, L, spin) as sched:
        got, _ = run_operator(case, realloc=True)
    report(f"A' {case}", us, n, spin, sched.injected_us)
    compare(f"A' {case} under slow_side with reallocation pressure", ref, got)


def test_control_without_the_join_the_delayed_gradient_is_seen_missing(monkeypatch):
    """Run once.  With ``ops._schedule_join`` doing nothing, a device-side clone of the attached weight gradient on the main stream,
    before any synchronisation, must NOT be the one_stream gradient: the weight-gradient GEMM sits behind the spin.  Only live,
    persistent buffers are touched: a value race, not a fault.
    The second assertion -- the clone still holds the buffer's start value, so it is the spin that kept the GEMM away -- depends on
    timing: the last side launch (net.0.weight) sits behind spins worth twice the undelayed pass, a margin of about one undelayed pass
    over the main stream; a stall of the host in this run that the reference run did not have could use it up with no ordering bug
    present.  The message says which of the two it was."""
    case = "doubleconv"
    ref, us, n = operator_reference(case)
    require_overlap()
    spin = SO.plan_spin(us, n)
    monkeypatch.setattr(ops, "_schedule_join", lambda device: None)
    with ops.deterministic(), SO.slow_side(ops, L, spin) as sched:
        got, _ = run_operator(case, after_backward=lambda params, start: {w + k: t.detach().clone() for k, p in params if k.endswith("net.0.weight")
                                                                          for w, t in (("early ", p.grad), ("start ", start[k]))})
    torch.cuda.synchronize()
    report(f"E {case}", us, n, spin, sched.injected_us)
    early = [k for k in got if k.startswith("early ")]
    assert len(early) == 1
    name = early[0][len("early "):]
    differs = not same(got[early[0]], ref[name])
    print(f"[stream order] E control: the un-joined clone of {name} differs from the one_stream gradient: {differs}")
    assert differs, "the schedule has no power: without the join the main stream still saw the finished weight gradient"
    # ... and it is the spin that did it: the clone holds the buffer's start value, the side GEMM had not begun behind its spins
    untouched = same(got[early[0]], got["start " + name])
    print(f"[stream order] E control: the un-joined clone still holds the start value of the buffer: {untouched}")
    assert untouched, "the un-joined clone is neither the finished gradient nor the start value: the side work was under way"
    # after the synchronisation the buffers themselves are complete, as ever
    compare("E after synchronisation", ref, {k: v for k, v in got.items() if not k.startswith(("early ", "start "))})


# ---------------------------------------------------------------------------------------------
# B. steps
# ---------------------------------------------------------------------------------------------
STEPS = 3
LR, WD = 1e-3, 1e-4


def build_unet(base, B, T, hw):
    torch.manual_seed(5)
    model = U.TemporalUNetDualView(1, 1, base_ch=base, use_skip_lstm=True).to(DEV).train()
    d = U.SyntheticSequences(B, T, hw, hw, seed=6, kind="uniform")
    return model, (d.x, d.y, d.mask)


def build_resnet():
    B, T, H, W, layers = 2, 2, 64, 64, 1          # the smallest case of tests/test_gpu_resnet_unfrozen.py
    model = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=layers).to(DEV)
    model.load_state_dict(RC.make_state(100 + layers, 1, layers), strict=True)
    model.unfreeze_encoder("all").train()
    return model, tuple(t.to(DEV) for t in RC.make_batch(200 + H + W, B, T, H, W))


STEP_CONFIGS = {
    "unet8-bf16": (lambda: build_unet(8, 2, 3, 32), False, True),
    "unet8-fp16": (lambda: build_unet(8, 2, 3, 32), True, True),
    "unet8-bf16-panel-by-panel": (lambda: build_unet(8, 2, 3, 32), False, False),
    "unet64-bf16": (lambda: build_unet(**LARGE), False, True),
    "resnet18-unfrozen-bf16": (build_resnet, False, True),
}


def run_steps(model, state, batch, fp16, schedule):
    """STEPS train_steps from ``state`` with NO synchronisation between them; after each a device-side snapshot on the main stream
    (loss, flat_g, flat_p, m, v, sumsq, every buffer), after the last an evaluation-mode forward.  ``schedule(k)`` is called
    after step k (hand-off counts per step).  -> (snapshots, device time of each step in us)."""
    ops.prepack_end()
    ops._PACK_PLAN.clear()
    model.load_state_dict(state)
    model.train()
    opt = U.FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=1.0, **(dict(loss_scale=2.0 ** 14) if fp16 else {}))
    x, y, mask = batch
    events = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
    snaps = []
    torch.cuda.synchronize()
    events[0].record()
    for k in range(STEPS):
        loss, _ = U.train_step(model, opt, x, y, mask, True)
        events[k + 1].record()
        snaps.append(TL.snapshot(model, opt, loss, sumsq=opt.sumsq))
        schedule(k)
    model.eval()
    with torch.no_grad():
        out, _ = model(x)
        snaps[-1]["eval forward"] = (out.stacked if hasattr(out, "stacked") else out).detach().clone()
    model.train()
    torch.cuda.synchronize()
    return snaps, [events[k].elapsed_time(events[k + 1]) * 1e3 for k in range(STEPS)]


@pytest.mark.parametrize("config", list(STEP_CONFIGS))
def test_three_steps_under_every_schedule(config):
    build, fp16, batched = STEP_CONFIGS[config]
    dev = device()
    with ops.deterministic(), ops.compute_dtype(torch.float16 if fp16 else torch.bfloat16):
        ops.PACK_BATCHED = batched
        model, batch = build()
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        names, sizes = TL.layout(model)
        per_step = {"side": [], "main": []}

        def counting(side, main):
            seen = [0, 0]

            def after(k):
                per_step["side"].append(side.handoffs - seen[0])
                per_step["main"].append(main.handoffs - seen[1])
                seen[:] = [side.handoffs, main.handoffs]
            return after

        with SO.one_stream(ops, dev), SO.both(ops, L, U.FusedAdamW) as (side, main):
            ref, times = run_steps(model, state, batch, fp16, counting(side, main))
        us = sorted(times)[len(times) // 2]
        n_side, n_main = min(per_step["side"]), min(per_step["main"])          # (the first step has no look-ahead pack)
        assert n_side >= 2 and n_main == 2, (per_step, "weight gradients, BatchNorm work and the look-ahead pack go to the side stream")
        assert bool(torch.isfinite(ref[-1]["loss"])) and not same(ref[0]["flat_p"], ref[-1]["flat_p"])
        require_overlap()
        side_spin, main_spin = SO.plan_spin(us, n_side), SO.plan_spin(us, n_main)
        print(f"[stream order] B {config}: undelayed steps {[round(t) for t in times]} us (median {us:.0f}), hand-offs per step "
              f"side {per_step['side']} main {per_step['main']}")
        for name in SO.SCHEDULES[1:]:
            spins = (side_spin if name != "slow_main" else SO.Spin(), main_spin if name != "slow_side" else SO.Spin())
            with SO.both(ops, L, U.FusedAdamW, *spins) as (side, main):
                got, _ = run_steps(model, state, batch, fp16, lambda k: None)
            if spins[0].us:
                report(f"B {config} {name}", us * STEPS, side.handoffs, side_spin, side.injected_us, "side")
            if spins[1].us:
                report(f"B {config} {name}", us * STEPS, main.handoffs, main_spin, main.injected_us, "main")
            for k in range(STEPS):
                compare(f"B {config} under {name}, step {k}", ref[k], got[k], names, sizes)
            del got
        del ref, model, state


# ---------------------------------------------------------------------------------------------
# C. graph (child process: tests/test_gpu_deterministic.py on captured graphs per process)
# ---------------------------------------------------------------------------------------------
def graph_child():
    ops.set_deterministic(True)
    dev = device()
    out = dict(steps=[], overlap=None)

    def make():
        torch.manual_seed(5)
        m = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV).train()
        o = U.FusedAdamW(m.parameters(), lr=LR, weight_decay=WD, max_grad_norm=1.0, capturable=True)
        return m, o

    d = U.SyntheticSequences(2, 3, 32, 32, seed=6, kind="uniform")
    # the undelayed step, measured on a model of its own.  A capture keeps the running statistics on the capturing stream
    # (ops._bn_forward_stats), so those hand-offs of the eager step are not counted
    probe, oprobe = make()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with SO.one_stream(ops, dev), SO.slow_side(ops, L) as count:
        for k in range(3):
            if k == 2:
                before = count.handoffs - count.by_name.get("running_stats", 0)
                torch.cuda.synchronize()
                e0.record()
            U.train_step(probe, oprobe, d.x, d.y, d.mask, True)
        e1.record()
        torch.cuda.synchronize()
    us, n = e0.elapsed_time(e1) * 1e3, count.handoffs - count.by_name.get("running_stats", 0) - before
    del probe, oprobe
    ops.prepack_end()
    ops._PACK_PLAN.clear()
    main, side = torch.cuda.current_stream(), ops.side_stream(dev)
    out["overlap"] = bool(side != main and overlap(main, side))
    if not out["overlap"]:
        return out
    spin = SO.plan_spin(us, n)
    m8, o8 = make()
    with SO.slow_side(ops, L, spin) as sched:
        g = U.GraphedTrainStep(m8, o8, d.x, d.y, d.mask, True, warmup=2)
    captured = sched.captured
    out.update(step_us=us, handoffs=n, spin=[spin.reps, spin.us], captured_handoffs=captured, injected_per_replay_us=captured * spin.per_handoff_us)
    twin, otwin = make()
    twin.load_state_dict(m8.state_dict())
    for a, b in ((otwin.m, o8.m), (otwin.v, o8.v), (otwin.hyper, o8.hyper)):
        a.copy_(b)
    names, sizes = TL.layout(m8)
    ops.prepack_end()
    ops._PACK_PLAN.clear()
    for k in range(3):
        lg, _ = g(d.x, d.y, d.mask)
        with SO.one_stream(ops, dev):
            le, _ = U.train_step(twin, otwin, d.x, d.y, d.mask, True)
        torch.cuda.synchronize()
        a = TL.snapshot(m8, o8, lg, step_count=o8.hyper[6:7], sumsq=o8.sumsq)
        b = TL.snapshot(twin, otwin, le, step_count=otwin.hyper[6:7], sumsq=otwin.sumsq)
        out["steps"].append(dict(diff=TL.first_difference(b, a, names, sizes), loss=float(lg), finite=bool(torch.isfinite(lg))))
    return out


def test_a_step_captured_under_a_delayed_side_stream_equals_eager_one_stream_steps():
    r = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[stream order] C graph child: {got}")
    assert got["overlap"], "the side stream does not run concurrently with the main stream: the captured spins delay nothing"
    assert got["spin"][1] <= SO.MAX_SPIN_US and got["captured_handoffs"] >= 2
    assert got["injected_per_replay_us"] >= SO.MIN_TOTAL_FACTOR * got["step_us"], got
    assert len(got["steps"]) == 3 and len({s["loss"] for s in got["steps"]}) == 3
    for k, s in enumerate(got["steps"]):
        assert s["finite"] and s["diff"] is None, f"replay {k} differs from the eager one_stream step: first differing tensor {s['diff']}"


# ---------------------------------------------------------------------------------------------
# D. FlatDDP, one rank over RCCL
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_group():
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29679")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV, 0))
        created = True
    yield
    if created:
        dist.destroy_process_group()


@pytest.mark.parametrize("grad_dtype", [None, torch.bfloat16], ids=["f32-buckets", "bf16-staging"])
def test_flat_ddp_buckets_wait_for_the_delayed_side_stream(one_rank_group, grad_dtype):
    """With staging a bucket copied before the side stream's accumulation is visible at world size 1: finalize() copies the stale
    stage back over flat_g.  Two steps, lr > 0, no synchronisation between them."""
    dev = device()
    data = U.SyntheticSequences(2, 3, 32, 32, seed=5, kind="blobs")

    def run(after_step):
        torch.manual_seed(77)
        model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV).train()
        opt = U.FusedAdamW(model.parameters(), lr=LR, weight_decay=0.0, max_grad_norm=None)
        ddp = U.FlatDDP(model, opt.flat, bucket_mb=0.05, grad_dtype=grad_dtype)
        ops.prepack_end()
        ops._PACK_PLAN.clear()
        snaps = []
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        try:
            assert len(ddp.buckets) > 3
            torch.cuda.synchronize()
            e[0].record()
            for k in range(2):
                loss, _ = U.train_step(model, opt, data.x, data.y, None, False, ddp, clip_norm=None)
                e[k + 1].record()
                snaps.append(TL.snapshot(model, opt, loss))
                after_step(k)
            torch.cuda.synchronize()
        finally:
            ddp.remove_hooks()
        return snaps, TL.layout(model), [e[k].elapsed_time(e[k + 1]) * 1e3 for k in range(2)]

    with ops.deterministic():
        counts = []
        with SO.one_stream(ops, dev), SO.slow_side(ops, L) as count:
            ref, (names, sizes), times = run(lambda k: counts.append(count.handoffs))
        us, n = times[1], min(counts[0], counts[1] - counts[0])          # (the first step has no look-ahead pack)
        assert n >= 2 and float(ref[0]["flat_g"].abs().max()) > 0
        require_overlap()
        # the launch stream of the delayed run is one probed against the REAL side stream (one_stream drops a pick made inside it): on
        # a shared hardware queue the bucket copy would be ordered behind the side stream's spins with or without launch.wait_stream(side)
        main, side = torch.cuda.current_stream(), ops.side_stream(dev)
        launch = ops.launch_stream(dev, main)
        assert launch not in (main, side) and overlap(main, launch) and overlap(side, launch), \
            "FlatDDP's launch stream does not run concurrently with the main and the side stream: the delayed run would prove nothing"
        spin = SO.plan_spin(us, n)
        with SO.slow_side(ops, L, spin) as sched:
            got, _, _ = run(lambda k: None)
        report(f"D FlatDDP {'bf16 staging' if grad_dtype is not None else 'f32 buckets'}", us * 2, sched.handoffs, spin, sched.injected_us)
        for k in range(2):
            compare(f"D FlatDDP step {k} under slow_side", ref[k], got[k], names, sizes)


if __name__ == "__main__":
    print(json.dumps(graph_child()))
