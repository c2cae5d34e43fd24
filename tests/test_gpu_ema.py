"""Weight EMA on the device (GPU): uclstm_ema_update and uclstm_swap_f32 at the C ABI against the f64 restatement of
tests/ema_cases.py, then FusedAdamW.attach_ema through every branch of step(), a skipped fp16 step, WeightEMA.swapped(),
evaluate inside it and evaluate_report(ema=), checkpoints, and the captured step (in a child process: this file as a script, as tests/test_gpu_deterministic.py
runs its graph)."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (run as a script by the last test: this puts the repository root on sys.path)
import ema_cases as E

pytestmark = pytest.mark.gpu

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops
from unet_convlstm_amd.engine import _stack

DEV = "cuda"
GEO = E.kernel_constants()
SIZES = E.abi_sizes(GEO)
MID = SIZES[4]                                     # a full chunk and a partial one, two blocks


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _update(ema, p, state, sumsq=None):
    L.check(L.lib.uclstm_ema_update(_ptr(ema), _ptr(p), ema.numel(), _ptr(sumsq), _ptr(state), ops._stream()), "ema_update")
    torch.cuda.synchronize()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_update(got, e0, p, state0, sumsq, what):
    """One call against the restatement: the shadow within the bound (bit for bit the old one where nothing was due), the state
    bit for bit.  Returns the new host state."""
    want, state1, d = E.ema_ref(e0, p, state0, sumsq)
    shadow, state = got
    assert state.cpu().numpy().tobytes() == state1.tobytes(), f"{what}: state {state.tolist()} != {state1.tolist()}"
    if d is None:
        assert np.array_equal(shadow.cpu().numpy().view(np.int32), e0.view(np.int32)), f"{what}: the shadow moved on a step without an update"
        return state1
    bad, worst = E.violations(shadow.cpu().numpy(), want, e0, p)
    print(f"[ema] {what}: d = {float(d):.9g}, {bad} of {e0.size} elements outside 3 * 2^-24 * (|ema| + |p|), worst |err| / bound {worst:.3f}")
    assert bad == 0, f"{what}: {bad} elements outside the bound, worst ratio {worst}"
    return state1


# ---------------------------------------------------------------------------------------------
# A. the C ABI
# ---------------------------------------------------------------------------------------------
def test_sizes_reach_the_paths_they_are_meant_for():
    assert E.grid_blocks(SIZES[-1], GEO) == GEO["GRID_CAP"] and E.trips_of_block0(SIZES[-1], GEO) == 2


@pytest.mark.parametrize("kind", E.VALUE_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_one_update_against_f64(n, kind):
    e0, p = E.values(kind, n, seed=n % 1000)
    state0 = E.make_state(0.999, 10.0, 1, seen=5, done=5)
    ema, state = _dev(e0), _dev(state0)
    _update(ema, _dev(p), state)
    _check_update((ema, state), e0, p, state0, None, f"n={n} {kind}")
    if kind == "equal":
        assert np.array_equal(ema.cpu().numpy().view(np.int32), p.view(np.int32))          # ema == p stays exactly p


def test_subnormal_pairs_are_rounded_once_and_not_flushed():
    """Both operands subnormal: every f64 intermediate is exact, so the device must return the f64 result rounded to f32."""
    e0, p = E.values("both_subnormal", MID, seed=3)
    state0 = E.make_state(0.9, 0.0, 1)
    ema, state = _dev(e0), _dev(state0)
    _update(ema, _dev(p), state)
    want, _, d = E.ema_ref(e0, p, state0)
    assert d == np.float32(0.9)
    got = ema.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))
    assert np.count_nonzero(got) > 0.99 * MID                                             # not flushed to zero


@pytest.mark.parametrize("schedule", E.SCHEDULES, ids=lambda s: "decay%g-warmup%g-every%d" % s)
def test_updates_in_a_row_follow_the_counts(schedule):
    """Seven calls from the device's own previous shadow with fresh weights each time.  Element 0 is a probe: ema = 1, p = 0
    makes the new value d itself, so the decay of every update is compared EXACTLY with the restatement's."""
    rng = np.random.default_rng(7)
    state_h = E.make_state(*schedule)
    e_h = rng.standard_normal(MID).astype(np.float32)
    ema, state = _dev(e_h), _dev(state_h)
    updates = 0
    for call in range(7):
        ema[0] = 1.0
        e_h = ema.cpu().numpy()
        p_h = rng.standard_normal(MID).astype(np.float32)
        p_h[0] = 0.0
        d = E.decay_of(state_h)
        due = E.ema_ref(e_h, p_h, state_h)[2] is not None
        _update(ema, _dev(p_h), state)
        state_h = _check_update((ema, state), e_h, p_h, state_h, None, f"{schedule} call {call}")
        probe = float(ema[0].item())
        assert probe == (float(d) if due else 1.0), f"{schedule} call {call}: decay {probe!r}, restatement {float(d)!r}"
        updates += due
    assert state_h[E.I_SEEN] == 7 and state_h[E.I_DONE] == updates == (7 // schedule[2])
    assert updates >= 2


@pytest.mark.parametrize("ss,skipped", E.SUMSQ_CASES + [(None, False)], ids=["inf", "nan", "finite", "null"])
def test_a_skipped_step_touches_nothing(ss, skipped):
    e0, p = E.values("random", MID, seed=11)
    state0 = E.make_state(0.9, 2.0, 1, seen=3, done=3)
    ema, state = _dev(e0), _dev(state0)
    sumsq = None if ss is None else torch.tensor([ss], dtype=torch.float64, device=DEV)
    _update(ema, _dev(p), state, sumsq)
    assert E.overflowed(ss) == skipped if ss is not None else not skipped
    if skipped:
        assert np.array_equal(ema.cpu().numpy().view(np.int32), e0.view(np.int32))
        assert state.cpu().numpy().tobytes() == state0.tobytes()                            # all eight floats
    else:
        s1 = _check_update((ema, state), e0, p, state0, ss, f"sumsq={ss}")
        assert s1[E.I_SEEN] == 4 and s1[E.I_DONE] == 4 and not np.array_equal(ema.cpu().numpy(), e0)
    if sumsq is not None:
        assert np.array_equal(sumsq.cpu().numpy().view(np.int64), np.array([ss], dtype=np.float64).view(np.int64))      # read only


@pytest.mark.parametrize("n", SIZES)
def test_swap_is_bit_exact_and_stays_inside_its_ranges(n):
    G = 64                                         # guard elements on both sides of both buffers
    rng = np.random.default_rng(n % 1000)
    host = rng.integers(-2 ** 31, 2 ** 31, 2 * (n + 2 * G), dtype=np.int64).astype(np.int32)      # any bit pattern, NaNs included
    buf = _dev(host).view(torch.float32)
    a, b = buf[G:G + n], buf[n + 3 * G:2 * n + 3 * G]
    L.check(L.lib.uclstm_swap_f32(_ptr(a), _ptr(b), n, ops._stream()), "swap_f32")
    torch.cuda.synchronize()
    want = host.copy()
    want[G:G + n], want[n + 3 * G:2 * n + 3 * G] = host[n + 3 * G:2 * n + 3 * G], host[G:G + n]
    got = buf.view(torch.int32).cpu().numpy()
    assert np.array_equal(got, want), "swap: contents or guards differ"
    L.check(L.lib.uclstm_swap_f32(_ptr(a), _ptr(b), n, ops._stream()), "swap_f32")
    torch.cuda.synchronize()
    assert np.array_equal(buf.view(torch.int32).cpu().numpy(), host), "swapping twice does not restore the buffers"
    if n >= 2:                                     # one element apart, n long: overlapping, refused, nothing written
        assert L.lib.uclstm_swap_f32(_ptr(a), _ptr(buf[G + 1:]), n, ops._stream()) == -1
        assert L.lib.uclstm_swap_f32(_ptr(buf[G + 1:]), _ptr(a), n, ops._stream()) == -1
        torch.cuda.synchronize()
        assert np.array_equal(buf.view(torch.int32).cpu().numpy(), host)


# ---------------------------------------------------------------------------------------------
# B. through the optimiser: every branch of step()
# ---------------------------------------------------------------------------------------------
FROZEN = "temporal.layers.0.conv.weight"
DATA = dict(B=2, T=2, hw=32)
BRANCHES = ("plain", "capturable", "fp16_scaled", "groups_frozen")


def _model():
    torch.manual_seed(5)
    return U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV).train()


def _data():
    return U.SyntheticSequences(DATA["B"], DATA["T"], DATA["hw"], DATA["hw"], seed=6, kind="uniform")


def _dtype(branch):
    return torch.float16 if branch == "fp16_scaled" else torch.bfloat16


def _build(branch):
    model = _model()
    if branch == "groups_frozen":
        dict(model.named_parameters())[FROZEN].requires_grad_(False)
        ps = [p for p in model.parameters() if p.requires_grad]
        groups = [dict(params=[p for p in ps if p.ndim > 1], weight_decay=1e-4), dict(params=[p for p in ps if p.ndim <= 1], weight_decay=0.0)]
        opt = U.FusedAdamW(groups, lr=1e-3, max_grad_norm=1.0, order=model.parameters())
        assert opt.uses_groups and opt.scale_state is None
    elif branch == "fp16_scaled":
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, loss_scale=2.0 ** 14)
        assert opt.scale_state is not None and not opt.uses_groups
    else:
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, capturable=branch == "capturable")
        assert not opt.uses_groups and opt.scale_state is None and opt.capturable == (branch == "capturable")
    return model, opt


def _follow(opt, ema, step_fn, what):
    """Run ``step_fn`` (one optimiser step) and check what it did to the EMA from the device's own previous shadow, new weights
    and sum of squares."""
    e0, s0 = ema.shadow.cpu().numpy(), ema.state.cpu().numpy()
    out = step_fn()
    torch.cuda.synchronize()
    ss = float(opt.sumsq.item()) if opt.scale_state is not None else None
    _check_update((ema.shadow, ema.state), e0, opt.flat.flat_p.cpu().numpy(), s0, ss, what)
    return out


def _run(branch, with_ema, steps=4):
    d = _data()
    with ops.deterministic(), ops.compute_dtype(_dtype(branch)):
        model, opt = _build(branch)
        ema = opt.attach_ema(decay=0.9, warmup=2.0, every=2 if branch == "groups_frozen" else 1) if with_ema else None
        losses = []
        for s in range(steps):
            step = lambda: U.train_step(model, opt, d.x, d.y, d.mask, True)[0]          # noqa: E731
            ops.LAUNCH_LOG = [] if s == steps - 1 else None                             # the launch log of the last step
            try:
                loss = _follow(opt, ema, step, f"{branch} step {s + 1}") if with_ema else step()
                log = ops.LAUNCH_LOG
            finally:
                ops.LAUNCH_LOG = None
            losses.append(loss.cpu().clone())
        torch.cuda.synchronize()
    out = dict(loss=torch.stack(losses), p=opt.flat.flat_p.cpu().clone(), m=opt.m.cpu().clone(), v=opt.v.cpu().clone(), log=log)
    return out, model, opt, ema


@pytest.mark.parametrize("branch", BRANCHES)
def test_every_branch_of_step_updates_the_shadow_and_nothing_else(branch):
    with_ema, model, opt, ema = _run(branch, True)
    every = 2 if branch == "groups_frozen" else 1
    applied = opt.steps_done()                     # 4, unless fp16 loss scaling skipped one (the EMA then has not seen it either)
    assert applied == 4 or (branch == "fp16_scaled" and 1 <= applied < 4)
    assert ema.steps_seen() == applied and ema.updates_done() == applied // every
    assert ema.shadow.numel() == opt.flat.numel == sum(p.numel() for p in model.parameters() if p.requires_grad)
    if branch == "groups_frozen":
        assert ema.shadow.numel() < sum(p.numel() for p in model.parameters())           # the frozen weight is not in the shadow
    assert not torch.equal(ema.shadow, opt.flat.flat_p) and bool(torch.isfinite(with_ema["loss"]).all())
    plain, *_ = _run(branch, False)
    for key in ("loss", "p", "m", "v"):
        assert _same_bits(with_ema[key], plain[key]), f"{branch}: the run with an EMA differs from the run without in {key}"
    # one more launch at the end of step(), with the sum of squares exactly where the branch can skip a step; nothing else moves
    assert [e for e in with_ema["log"] if e[0] == "ema"] == [("ema", "update", branch == "fp16_scaled")] == with_ema["log"][-1:]
    assert [e for e in with_ema["log"] if e[0] != "ema"] == plain["log"] and plain["log"]


def test_an_overflowed_fp16_step_is_not_averaged_in():
    """The third step's flat gradient gets one inf before step(): parameters, shadow and both counts stay, the fourth step
    updates again.  Decided on the device: nothing here tells the EMA about the overflow."""
    d = _data()
    with ops.deterministic(), ops.compute_dtype(torch.float16):
        model, opt = _build("fp16_scaled")
        ema = opt.attach_ema(decay=0.9, warmup=2.0)

        def step(poison):
            opt.zero_grad()
            out, _ = model(d.x)
            loss = U.compute_loss(_stack(out), d.y, d.mask, True)
            opt.scale_loss(loss).backward()
            if poison:
                opt.flat.flat_g[17] = float("inf")
            opt.step()

        for s in (1, 2):
            _follow(opt, ema, lambda: step(False), f"overflow run, step {s}")
        p, shadow, state = opt.flat.flat_p.clone(), ema.shadow.clone(), ema.state.clone()
        _follow(opt, ema, lambda: step(True), "overflow run, step 3 (overflowed)")
        assert not bool(torch.isfinite(opt.sumsq).all())
        assert _same_bits(opt.flat.flat_p, p) and _same_bits(ema.shadow, shadow) and _same_bits(ema.state, state)
        assert ema.steps_seen() == 2 == opt.steps_done() and ema.updates_done() == 2 and opt.step_count == 3
        _follow(opt, ema, lambda: step(False), "overflow run, step 4")
        assert ema.steps_seen() == 3 == opt.steps_done() and ema.updates_done() == 3 and not _same_bits(ema.shadow, shadow)


# ---------------------------------------------------------------------------------------------
# C. swapped(), model_state_dict(), evaluate(ema=)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    """The plain branch after three steps with a fast EMA (shadow and weights clearly apart), and a second model loaded from
    ema.model_state_dict: built once, left unchanged by the tests that share it."""
    d = _data()
    with ops.deterministic():
        model, opt = _build("plain")
        ema = opt.attach_ema(decay=0.5, warmup=0.0)
        for _ in range(3):
            U.train_step(model, opt, d.x, d.y, d.mask, True)
        second = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV)
        second.load_state_dict(ema.model_state_dict(model))
    torch.cuda.synchronize()
    return model, opt, ema, second, d


def _eval_forward(model, x):
    was = model.training
    model.eval()
    try:
        with torch.no_grad(), ops.deterministic():
            out, _ = model(x)
            y = _stack(out).float().clone()
    finally:
        model.train(was)
    torch.cuda.synchronize()
    return y


def test_swapped_computes_with_the_shadow_and_restores_the_weights(trained):
    model, opt, ema, second, d = trained
    p0, s0 = opt.flat.flat_p.clone(), ema.shadow.clone()
    ptrs = [p.data_ptr() for p in model.parameters()] + [p.grad.data_ptr() for p in opt.flat.params]
    assert not torch.equal(p0, s0)
    before = _eval_forward(model, d.x)
    want = _eval_forward(second, d.x)
    assert not torch.equal(before, want)                                  # the averaged weights predict something else
    epoch = ops.WEIGHTS_EPOCH
    with ema.swapped() as inside:
        assert inside is ema and ops.WEIGHTS_EPOCH == epoch + 1
        assert _same_bits(opt.flat.flat_p, s0) and _same_bits(ema.shadow, p0)
        got = _eval_forward(model, d.x)
    assert ops.WEIGHTS_EPOCH == epoch + 2
    assert _same_bits(got, want), "inside swapped() the model does not compute what the model loaded from model_state_dict computes"
    assert _same_bits(_eval_forward(model, d.x), before), "after swapped() the forward differs from the one before it"
    assert _same_bits(opt.flat.flat_p, p0) and _same_bits(ema.shadow, s0)
    assert ptrs == [p.data_ptr() for p in model.parameters()] + [p.grad.data_ptr() for p in opt.flat.params]      # no address moved
    # restored when the body raises, too
    with pytest.raises(ZeroDivisionError):
        with ema.swapped():
            1 / 0
    assert _same_bits(opt.flat.flat_p, p0) and _same_bits(ema.shadow, s0) and ops.WEIGHTS_EPOCH == epoch + 4


def test_swapped_refusals(trained):
    model, opt, ema, second, d = trained
    p0, s0, state0 = opt.flat.flat_p.clone(), ema.shadow.clone(), ema.state.clone()
    buffers0 = {k: b.detach().float().clone() for k, b in model.named_buffers()}
    with ema.swapped():
        with pytest.raises(RuntimeError, match="nest"):
            with ema.swapped():
                pass
        with pytest.raises(RuntimeError, match="swapped"):
            opt.step()
        with pytest.raises(RuntimeError, match="swapped"):
            U.train_step(model, opt, d.x, d.y, d.mask, True)
        with pytest.raises(RuntimeError, match="swapped"):
            ema.model_state_dict(model)
        with pytest.raises(RuntimeError, match="swapped"):
            opt.state_dict()
    torch.cuda.synchronize()
    assert _same_bits(opt.flat.flat_p, p0) and _same_bits(ema.shadow, s0) and _same_bits(ema.state, state0)
    # train_step refuses before its forward pass: BatchNorm's running statistics have not moved either
    assert all(_same_bits(b.float(), buffers0[k]) for k, b in model.named_buffers())
    with pytest.raises(RuntimeError, match="attached already"):
        opt.attach_ema()
    with pytest.raises(TypeError, match="WeightEMA"):
        U.evaluate_report(model, [], torch.device(DEV), None, ema=opt)
    with pytest.raises(TypeError):
        U.evaluate(model, [], torch.device(DEV), None, ema=ema)          # evaluate's signature is pinned: with ema.swapped(): evaluate(...)


def test_evaluate_with_ema_equals_evaluate_of_the_loaded_model(trained, tmp_path):
    """``evaluate`` inside ``ema.swapped()`` and ``evaluate_report(ema=ema)`` against ``evaluate`` of the model loaded from
    ``model_state_dict``, to the bits of the loss and the metrics (deterministic mode: ordered reductions)."""
    model, opt, ema, second, _ = trained
    rng = np.random.default_rng(0)
    N, T, H, W = 8, 2, 32, 32
    X = (rng.random((N, T, 2, H, W)) * 30).astype(np.float32)
    X[X < 6] = 0.0
    Y = np.tanh(X[:, :, :1] / 15.0 - 1.0).astype(np.float32) * 4.0
    path = tmp_path / "eval.npz"
    np.savez(path, X=X, Y=Y)
    ds = U.NPZSequenceDataset(str(path))
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)
    p0 = opt.flat.flat_p.clone()
    with ops.deterministic():
        live = U.evaluate(model, loader, torch.device(DEV), ds, use_mask=True)
        with ema.swapped():
            got = U.evaluate(model, loader, torch.device(DEV), ds, use_mask=True)
        want = U.evaluate(second, loader, torch.device(DEV), ds, use_mask=True)
        rep = U.evaluate_report(model, loader, torch.device(DEV), ds, use_mask=True, ema=ema)
        again = U.evaluate(model, loader, torch.device(DEV), ds, use_mask=True)
    model.train()
    second.train()
    as_bytes = lambda t: [np.float64(v).tobytes() for v in t]          # noqa: E731
    assert all(np.isfinite(v) for v in got) and as_bytes(got) == as_bytes(want), f"{got} vs {want}"
    assert as_bytes(rep[:4]) == as_bytes(want)
    assert as_bytes(live) != as_bytes(got) and as_bytes(again) == as_bytes(live)
    assert _same_bits(opt.flat.flat_p, p0)


# ---------------------------------------------------------------------------------------------
# D. checkpoints
# ---------------------------------------------------------------------------------------------
SHAPES = [(7, 3), (5,), (4, 2, 3, 3), (1,), (64,), (16, 8, 3, 3)]


def _tensor_optimiser(init, ema_args):
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = U.FusedAdamW(ps, lr=1e-2, weight_decay=1e-4, max_grad_norm=1.0)
    return ps, opt, (opt.attach_ema(*ema_args) if ema_args is not None else None)


def _tensor_step(ps, opt, grads):
    opt.zero_grad()
    for p, g in zip(ps, grads):
        p.grad.copy_(g)
    opt.step()


def test_state_dict_round_trip_continues_bit_for_bit():
    g = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(6)]
    args = (0.9, 3.0, 2)
    with ops.deterministic():
        ps, opt, ema = _tensor_optimiser(init, args)
        for k in range(3):
            _tensor_step(ps, opt, grads[k])
        sd = opt.state_dict()
        weights = [p.detach().clone() for p in ps]
        assert set(sd["fused"]["ema"]) == {"shadow", "state"} and sd["fused"]["ema"]["shadow"].data_ptr() != ema.shadow.data_ptr()
        assert ema.steps_seen() == 3 and ema.updates_done() == 1
        # a fresh optimiser over the saved weights, another EMA configuration: the saved one wins
        ps2, opt2, ema2 = _tensor_optimiser(weights, (0.5, 0.0, 1))
        opt2.load_state_dict(sd)
        assert _same_bits(ema2.shadow, ema.shadow) and _same_bits(ema2.state, ema.state)
        assert (ema2.decay, ema2.warmup, ema2.every) == (float(np.float32(0.9)), 3.0, 2)
        for k in range(3, 6):
            _tensor_step(ps, opt, grads[k])
            _tensor_step(ps2, opt2, grads[k])
        torch.cuda.synchronize()
        assert _same_bits(opt2.flat.flat_p, opt.flat.flat_p) and _same_bits(opt2.m, opt.m) and _same_bits(opt2.v, opt.v)
        assert _same_bits(ema2.shadow, ema.shadow) and _same_bits(ema2.state, ema.state)
        assert ema2.steps_seen() == 6 and ema2.updates_done() == 3
        # a state WITHOUT "ema" re-seeds the shadow from the weights as they are and zeroes the counts
        bare = {k: (dict((kk, vv) for kk, vv in v.items() if kk != "ema") if k == "fused" else v) for k, v in sd.items()}
        ps3, opt3, ema3 = _tensor_optimiser(weights, args)
        _tensor_step(ps3, opt3, grads[0])
        assert ema3.steps_seen() == 1
        opt3.load_state_dict(bare)
        assert _same_bits(ema3.shadow, opt3.flat.flat_p) and ema3.steps_seen() == 0 and ema3.updates_done() == 0
        assert ema3.state[:3].tolist() == [float(np.float32(0.9)), 3.0, 2.0]
        # a state WITH "ema" loaded into an optimiser without one: ignored
        ps4, opt4, none = _tensor_optimiser(weights, None)
        opt4.load_state_dict(sd)
        assert none is None and opt4.ema is None and "ema" not in opt4.state_dict()["fused"] and _same_bits(opt4.m, sd["fused"]["exp_avg"])


# ---------------------------------------------------------------------------------------------
# E. the captured step
# ---------------------------------------------------------------------------------------------
def graphed():
    """GraphedTrainStep with an EMA attached: counts after capture, the shadow replay by replay, swapped() between replays, the
    refusals under capture.  Returns what the parent asserts on."""
    out = {}
    d = _data()
    with ops.deterministic():
        model = _model()
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, capturable=True)
        ema = opt.attach_ema(decay=0.9, warmup=2.0)
        g = U.GraphedTrainStep(model, opt, d.x, d.y, d.mask, True, warmup=2)
        torch.cuda.synchronize()
        out["after_capture"] = [ema.steps_seen(), ema.updates_done(), opt.steps_done()]          # two eager warm-up steps; the capture ran nothing
        bad_total, worst = 0, 0.0
        for r in range(3):
            e0, s0 = ema.shadow.cpu().numpy(), ema.state.cpu().numpy()
            g(d.x, d.y, d.mask)
            torch.cuda.synchronize()
            want, s1, dk = E.ema_ref(e0, opt.flat.flat_p.cpu().numpy(), s0)
            bad, ratio = E.violations(ema.shadow.cpu().numpy(), want, e0, opt.flat.flat_p.cpu().numpy())
            bad_total, worst = bad_total + bad, max(worst, ratio)
            out.setdefault("state_ok", []).append(ema.state.cpu().numpy().tobytes() == s1.tobytes() and dk is not None)
        out["violations"], out["worst_ratio"] = bad_total, worst
        out["after_replays"] = [ema.steps_seen(), ema.updates_done(), opt.steps_done()]
        # a replay from a saved state, without and with swapped() (and an eval forward on the averaged weights) in front of it
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        saved = [t.detach().clone() for t in (opt.m, opt.v, opt.hyper, ema.shadow, ema.state)]

        def replay(swap):
            model.load_state_dict(state)
            for t, s in zip((opt.m, opt.v, opt.hyper, ema.shadow, ema.state), saved):
                t.copy_(s)
            if swap:
                with ema.swapped():
                    _eval_forward(model, d.x)
                    try:
                        g(d.x, d.y, d.mask)
                        out["replay_inside_swapped_refused"] = False
                    except RuntimeError:
                        out["replay_inside_swapped_refused"] = True
            loss, _ = g(d.x, d.y, d.mask)
            torch.cuda.synchronize()
            return [t.cpu().clone() for t in (loss, opt.flat.flat_p, opt.m, opt.v, ema.shadow, ema.state)]

        a, b = replay(False), replay(True)
        out["swap_between_replays_same_bits"] = [bool(_same_bits(x, y)) for x, y in zip(a, b)]
        out["moved"] = not _same_bits(a[1], saved[3]) and bool(torch.isfinite(a[0]))
        # under a capture: swapped() refuses before it launches anything
        t = torch.zeros(8, device=DEV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                t.add_(1.0)
                try:
                    with ema.swapped():
                        pass
                    out["swapped_under_capture_refused"] = False
                except RuntimeError as e:
                    out["swapped_under_capture_refused"] = "capture" in str(e)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        out["untouched_by_refusal"] = bool(_same_bits(ema.shadow, b[4]))
    return out


def test_graphed_step_carries_the_ema():
    r = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[ema] graphed step: {got}")
    assert got["after_capture"] == [2, 2, 2], got                 # the counts are the applied steps: warm-up yes, capture no
    assert got["after_replays"] == [5, 5, 5] and all(got["state_ok"]), got
    assert got["violations"] == 0, got
    assert all(got["swap_between_replays_same_bits"]) and got["moved"], got
    assert got["replay_inside_swapped_refused"] and got["swapped_under_capture_refused"] and got["untouched_by_refusal"], got


if __name__ == "__main__":
    print(json.dumps(graphed()))
