"""StepMonitor on the device (GPU): uclstm_param_stats at the C ABI against the f64 restatement of tests/monitor_cases.py, then
FusedAdamW.attach_monitor through every branch of step(), an overflowed fp16 step, names and groups, reseed() / load_state_dict,
and the captured step (in a child process: this file as a script, as tests/test_gpu_ema.py runs its graph)."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (run as a script by the last test: this puts the repository root on sys.path)
import monitor_cases as M

pytestmark = pytest.mark.gpu

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops
from unet_convlstm_amd.engine import _stack
from unet_convlstm_amd.optim import StepMonitor, build_stat_blocks, check_stat_blocks

DEV = "cuda"
CHUNK = M.chunk()
LAYOUT = M.abi_layout(CHUNK)
NAN_TENSOR = len(LAYOUT) - 1
GUARD = 64                                         # elements on both sides of every buffer: keeps the 16-byte alignment of the f32 buffers


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Guarded:
    """A device buffer with GUARD elements of a known pattern in front of it and behind it."""

    def __init__(self, host: np.ndarray):
        self.host = np.ascontiguousarray(host)
        flat = self.host.reshape(-1)
        fill = np.full(GUARD, 77, dtype=flat.dtype)
        self.whole = torch.from_numpy(np.concatenate([fill, flat, fill])).to(DEV)
        self.t = self.whole[GUARD:GUARD + flat.size]
        self.fill = fill

    def get(self) -> np.ndarray:
        return self.t.cpu().numpy().reshape(self.host.shape)

    def guards_intact(self) -> bool:
        w = self.whole.cpu().numpy()
        return bool(np.array_equal(w[:GUARD], self.fill) and np.array_equal(w[-GUARD:], self.fill))


class Call:
    """The buffers of one uclstm_param_stats set-up over ``sizes``, every one of them guarded, and their host mirrors."""

    def __init__(self, sizes, p, g, prev, every, history, seen=0, done=0):
        self.sizes, self.history, self.n = list(sizes), history, int(np.sum(sizes))
        blocks, tensors = build_stat_blocks(self.sizes, CHUNK)
        check_stat_blocks(blocks, tensors, self.n, CHUNK)
        self.p, self.g = Guarded(p), Guarded(g)
        self.prev = None if prev is None else Guarded(prev)
        self.blocks, self.tensors = Guarded(blocks), Guarded(tensors)
        self.partials = Guarded(np.full((blocks.shape[0], 8), -1.0))
        self.ring = Guarded(np.full((history, len(self.sizes), 8), -2.0))
        self.meta = Guarded(np.full((history, 4), -3.0))
        self.state = Guarded(M.make_state(every, seen, done))
        self.everything = [b for b in (self.p, self.g, self.prev, self.blocks, self.tensors, self.partials, self.ring, self.meta, self.state) if b is not None]

    def run(self, sumsq=None, scale=None):
        ss = None if sumsq is None else torch.tensor([sumsq], dtype=torch.float64, device=DEV)
        sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=DEV)
        L.check(L.lib.uclstm_param_stats(_ptr(self.p.t), _ptr(self.g.t), None if self.prev is None else _ptr(self.prev.t), self.n,
                                         _ptr(self.blocks.t), int(self.blocks.host.shape[0]), _ptr(self.tensors.t), len(self.sizes),
                                         _ptr(self.partials.t), _ptr(self.ring.t), _ptr(self.meta.t), self.history, _ptr(ss), _ptr(sc),
                                         _ptr(self.state.t), ops._stream()), "param_stats")
        torch.cuda.synchronize()

    def guards_intact(self) -> bool:
        return all(b.guards_intact() for b in self.everything)


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _check_rows(got, want, sizes, what):
    bad, over_half = M.compare_rows(got, want, sizes)
    print(f"[monitor] {what}: {len(sizes)} tensors, {len(bad)} values outside (count + 4) * 2^-53 * ref or unequal, "
          f"{over_half} tensors beyond half of the bound")
    assert not bad, f"{what}: (tensor, column, device, restatement) {bad[:8]}"


# ---------------------------------------------------------------------------------------------
# A. the C ABI
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    g, p, prev = M.planted(LAYOUT, CHUNK, seed=3, nan_tensor=NAN_TENSOR)
    want = {True: np.stack([M.tensor_ref(g[o:o + n], p[o:o + n], prev[o:o + n]) for o, n in zip(M.offsets_of(LAYOUT), LAYOUT)]),
            False: np.stack([M.tensor_ref(g[o:o + n], p[o:o + n]) for o, n in zip(M.offsets_of(LAYOUT), LAYOUT)])}
    return g, p, prev, want


@pytest.mark.parametrize("updates", [True, False], ids=["prev", "no-prev"])
def test_one_record_against_f64(planted, updates):
    g, p, prev, want = planted
    assert {int(o) % 4 for o in M.offsets_of(LAYOUT)} == {0, 1, 2, 3} and set(M.abi_sizes(CHUNK)) <= set(LAYOUT)
    c = Call(LAYOUT, p, g, prev if updates else None, every=1, history=3, seen=4, done=7)
    c.run(sumsq=2.5, scale=8.0)
    ring, meta, state = c.ring.get(), c.meta.get(), c.state.get()
    slot = 7 % 3
    _check_rows(ring[slot], want[updates], LAYOUT, f"planted layout, updates={updates}")
    assert ring[slot, NAN_TENSOR].tolist() == [0.0, 0.0, 7.0, 0.0, 0.0, 0.0, 7.0, 0.0]          # all NaN: sums 0, maxima 0
    if not updates:
        assert not ring[slot, :, 7].any()
    assert np.all(ring[[s for s in range(3) if s != slot]] == -2.0), "another slot of the ring was written"
    assert meta[slot].tolist() == [5.0, 8.0, 2.5, 0.0] and np.all(np.delete(meta, slot, axis=0) == -3.0)
    assert state.tolist() == [1, 5, 8, 1, slot, 0, 0, 0]
    # the inputs are read only, prev is p bit for bit, nothing outside any buffer moved
    assert np.array_equal(_bits(c.p.get()), _bits(p)) and np.array_equal(_bits(c.g.get()), _bits(g))
    if updates:
        assert np.array_equal(_bits(c.prev.get()), _bits(p)), "prev is not p bit for bit after a record"
    assert c.guards_intact()
    # the same call again on the same inputs: the same bits (no atomics, a fixed order)
    c2 = Call(LAYOUT, p, g, prev if updates else None, every=1, history=3, seen=4, done=7)
    c2.run(sumsq=2.5, scale=8.0)
    assert np.array_equal(_bits(c2.ring.get()), _bits(ring))


def test_a_call_that_does_not_record_touches_nothing_but_the_state(planted):
    g, p, prev, _ = planted
    c = Call(LAYOUT, p, g, prev, every=2, history=3, seen=0, done=1)
    c.run(sumsq=1.0, scale=2.0)
    assert c.state.get().tolist() == [2, 1, 1, 0, 1, 0, 0, 0]
    assert np.array_equal(_bits(c.prev.get()), _bits(prev)), "prev moved on a call that does not record"
    assert np.all(c.ring.get() == -2.0) and np.all(c.meta.get() == -3.0) and np.all(c.partials.get() == -1.0)
    assert np.array_equal(_bits(c.p.get()), _bits(p)) and np.array_equal(_bits(c.g.get()), _bits(g))
    assert c.guards_intact()
    c.run(sumsq=1.0, scale=2.0)                      # the second call is due
    assert c.state.get().tolist() == [2, 2, 2, 1, 1, 0, 0, 0] and c.meta.get()[1].tolist() == [2.0, 2.0, 1.0, 0.0]
    assert np.array_equal(_bits(c.prev.get()), _bits(p)) and c.guards_intact()


@pytest.mark.parametrize("sumsq,scale,skipped", M.META_CASES, ids=["null", "finite", "inf", "nan", "f64max"])
def test_meta_row_and_the_skipped_flag(sumsq, scale, skipped):
    sizes = [5, 3]
    rng = np.random.default_rng(0)
    p, g = rng.standard_normal(8).astype(np.float32), rng.standard_normal(8).astype(np.float32)
    c = Call(sizes, p, g, p.copy(), every=1, history=2)
    c.run(sumsq=sumsq, scale=scale)
    ring, meta, state, _, rec = M.call_ref(p, g, p, sizes, np.full((2, 2, 8), -2.0), np.full((2, 4), -3.0), M.make_state(1), 2, sumsq, scale)
    got = c.meta.get()
    assert rec and np.array_equal(_bits(got), _bits(meta)), (got, meta)
    assert got[0, 3] == float(skipped) and c.state.get().tolist() == state.tolist()
    _check_rows(c.ring.get()[0], ring[0], sizes, f"sumsq={sumsq}")
    assert not c.ring.get()[0, :, 7].any() and c.guards_intact()                          # prev == p: no update, exactly


def test_every_third_call_records_into_a_ring_of_two():
    sizes = [CHUNK + 1, 3, 2 * CHUNK - 1]
    n = sum(sizes)
    rng = np.random.default_rng(5)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    c = Call(sizes, p, g, p.copy(), every=3, history=2)
    ring, meta, state, prev = np.full((2, 3, 8), -2.0), np.full((2, 4), -3.0), M.make_state(3), p.copy()
    p_at = {}
    for call in range(1, 9):
        p = (p.astype(np.float64) + rng.standard_normal(n) * 1e-3).astype(np.float32)
        c.p.t.copy_(torch.from_numpy(p))
        c.run(sumsq=float(call))
        ring, meta, state, prev, rec = M.call_ref(p, g, prev, sizes, ring, meta, state, 2, float(call))
        p_at[call] = p
        assert rec == (call % 3 == 0) and c.state.get().tolist() == state.tolist(), call
        assert np.array_equal(_bits(c.prev.get()), _bits(prev)), f"call {call}: prev"
    assert state[M.I_SEEN] == 8 and state[M.I_DONE] == 2
    got = c.ring.get()
    assert np.array_equal(c.meta.get()[:, 0], [3.0, 6.0]) and np.array_equal(_bits(c.meta.get()), _bits(meta))
    for slot in (0, 1):
        _check_rows(got[slot], ring[slot], sizes, f"every=3 history=2, record {3 * (slot + 1)}")
    # the update column of record 6 is the change over calls 4..6
    over = np.stack([M.tensor_ref(g[o:o + k], p_at[6][o:o + k], p_at[3][o:o + k]) for o, k in zip(M.offsets_of(sizes), sizes)])
    assert np.array_equal(over[:, 7], ring[1][:, 7]) and (over[:, 7] > 0).all()
    r = StepMonitor.reduce(got, c.meta.get(), 2, 2)
    assert r["step"].tolist() == [3, 6] and c.guards_intact()


# ---------------------------------------------------------------------------------------------
# B. through the optimiser: every branch of step()
# ---------------------------------------------------------------------------------------------
FROZEN = "temporal.layers.0.conv.weight"
DATA = dict(B=2, T=2, hw=32)
BRANCHES = ("plain", "clipped", "capturable", "groups", "fp16_scaled", "fp16_scaled_groups")
# what step() hands to the record: (a global sum of squares, the loss scale in effect)
PASSES = {"plain": (False, False), "clipped": (True, False), "capturable": (True, False), "groups": (True, False),
          "fp16_scaled": (True, True), "fp16_scaled_groups": (True, True)}


def _model():
    torch.manual_seed(5)
    return U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV).train()


def _data():
    return U.SyntheticSequences(DATA["B"], DATA["T"], DATA["hw"], DATA["hw"], seed=6, kind="uniform")


def _dtype(branch):
    return torch.float16 if branch.startswith("fp16") else torch.bfloat16


def _build(branch):
    model = _model()
    if branch == "groups":
        dict(model.named_parameters())[FROZEN].requires_grad_(False)
        ps = [p for p in model.parameters() if p.requires_grad]
        groups = [dict(params=[p for p in ps if p.ndim > 1], weight_decay=1e-4), dict(params=[p for p in ps if p.ndim <= 1], weight_decay=0.0, lr=1e-4)]
        opt = U.FusedAdamW(groups, lr=1e-3, max_grad_norm=1.0, order=model.parameters())
        assert opt.uses_groups and opt.scale_state is None
    elif branch == "fp16_scaled":
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, loss_scale=2.0 ** 14)
        assert opt.scale_state is not None and not opt.uses_groups
    elif branch == "fp16_scaled_groups":
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, loss_scale=2.0 ** 14, capturable=True)
        assert opt.scale_state is not None and opt.uses_groups
    else:
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0 if branch != "plain" else None,
                           capturable=branch == "capturable")
        assert not opt.uses_groups and opt.scale_state is None and opt.capturable == (branch == "capturable")
    return model, opt


def _expected_record(opt, prev_h, passes):
    """The restatement's rows and meta values of the step that has just run, from host copies of the optimiser's buffers."""
    f = opt.flat
    p, g = f.flat_p.cpu().numpy(), f.flat_g.cpu().numpy()
    sizes = [q.numel() for q in f.params]
    rows = np.stack([M.tensor_ref(g[o:o + n], p[o:o + n], None if prev_h is None else prev_h[o:o + n]) for o, n in zip(f.offsets, sizes)])
    sumsq = float(opt.sumsq.item()) if passes[0] else None
    scale = float(opt._last_scale.item()) if passes[1] else None
    return rows, sumsq, scale


def _run(branch, with_monitor, steps=3, updates=True):
    d = _data()
    records = []
    with ops.deterministic(), ops.compute_dtype(_dtype(branch)):
        model, opt = _build(branch)
        mon = opt.attach_monitor(every=1, history=4, updates=updates, names=model.named_parameters()) if with_monitor else None
        for s in range(steps):
            prev_h = mon.prev.cpu().numpy() if (mon is not None and updates) else None
            ops.LAUNCH_LOG = [] if s == steps - 1 else None                             # the launch log of the last step
            try:
                # train_step hands its clip_norm to the optimiser: None keeps the plain branch free of a global norm
                U.train_step(model, opt, d.x, d.y, d.mask, True, clip_norm=None if branch == "plain" else 1.0)
                log = ops.LAUNCH_LOG
            finally:
                ops.LAUNCH_LOG = None
            torch.cuda.synchronize()
            if mon is not None:
                records.append(_expected_record(opt, prev_h, PASSES[branch]))
        torch.cuda.synchronize()
    out = dict(p=opt.flat.flat_p.cpu().clone(), m=opt.m.cpu().clone(), v=opt.v.cpu().clone(), log=log)
    return out, model, opt, mon, records


def _same_bits(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


@pytest.mark.parametrize("branch", BRANCHES)
def test_every_branch_of_step_records_and_changes_nothing_else(branch):
    with_mon, model, opt, mon, records = _run(branch, True)
    sizes = [q.numel() for q in opt.flat.params]
    assert mon.steps_seen() == 3 == mon.records_done()
    ring, meta = mon.ring.cpu().numpy(), mon.meta.cpu().numpy()
    r = mon.read()
    assert r["step"].tolist() == [1, 2, 3] and r["names"] == mon.names and r["numel"].tolist() == sizes
    for k, (rows, sumsq, scale) in enumerate(records):
        _check_rows(ring[k], rows, sizes, f"{branch} step {k + 1}")
        want_meta = np.array([k + 1.0, 1.0 if scale is None else scale, np.nan if sumsq is None else sumsq,
                              float(sumsq is not None and M.overflowed(sumsq))])
        assert np.array_equal(_bits(meta[k]), _bits(want_meta)), (branch, k, meta[k], want_meta)
        s = 1.0 if scale is None else scale
        np.testing.assert_allclose(r["grad_norm"][k], np.sqrt(rows[:, 0]) / s, rtol=1e-10, atol=0)
        np.testing.assert_allclose(r["update_norm"][k], np.sqrt(rows[:, 7]), rtol=1e-10, atol=0)
        assert np.array_equal(r["grad_max"][k], rows[:, 1] / s) and np.array_equal(r["weight_max"][k], rows[:, 5])
        assert np.array_equal(r["grad_nonfinite"][k], rows[:, 2]) and np.array_equal(r["grad_zero_frac"][k], rows[:, 3] / np.asarray(sizes))
        if sumsq is None:
            assert np.isnan(r["global_grad_norm"][k])
        else:
            assert r["global_grad_norm"][k] == np.sqrt(sumsq) / s
            if not r["skipped"][k]:                 # the per-tensor norms add up to the optimiser's own global norm
                np.testing.assert_allclose(np.sqrt(np.sum(r["grad_norm"][k] ** 2)), r["global_grad_norm"][k], rtol=1e-5)
    applied = ~r["skipped"]
    assert applied.any() and (r["update_norm"][applied] > 0).any() and not r["update_norm"][~applied].any()
    # read() is reduce() of the raw buffers
    again = StepMonitor.reduce(ring, meta, 3, 4, True, mon.names, mon.numel, mon.group)
    assert all(np.array_equal(r[key], again[key], equal_nan=True) for key in StepMonitor.PER_TENSOR + ("step", "scale", "global_grad_norm"))
    # the same run without a monitor: the same bits, and the same launches but for the record at the end of step()
    plain, *_ = _run(branch, False)
    for key in ("p", "m", "v"):
        assert _same_bits(with_mon[key], plain[key]), f"{branch}: the run with a monitor differs from the run without in {key}"
    assert [e for e in with_mon["log"] if e[0] == "monitor"] == [("monitor", "stats") + PASSES[branch]] == with_mon["log"][-1:]
    assert [e for e in with_mon["log"] if e[0] != "monitor"] == plain["log"] and plain["log"]
    assert not any(e[0] == "monitor" for e in plain["log"])


def test_without_updates_no_copy_is_held_and_the_columns_read_nan():
    _, model, opt, mon, records = _run("clipped", True, steps=2, updates=False)
    assert mon.prev is None
    r = mon.read()
    assert np.isnan(r["update_norm"]).all() and np.isnan(r["update_ratio"]).all() and r["step"].tolist() == [1, 2]
    sizes = [q.numel() for q in opt.flat.params]
    for k, (rows, _, _) in enumerate(records):
        _check_rows(mon.ring.cpu().numpy()[k], rows, sizes, f"updates=False step {k + 1}")
    assert "largest" not in mon.report() and "group 0" in mon.report()


def test_names_and_groups_follow_the_model_and_the_optimiser():
    with ops.compute_dtype(torch.bfloat16):
        model, opt = _build("groups")
        mon = opt.attach_monitor(names=model.named_parameters())
        by_id = {id(p): n for n, p in model.named_parameters()}
        assert mon.names == [by_id[id(p)] for p in opt.flat.params] and FROZEN not in mon.names
        group_of = {id(p): gi for gi, g in enumerate(opt.param_groups) for p in g["params"]}
        assert mon.group.tolist() == [group_of[id(p)] for p in opt.flat.params] and set(mon.group.tolist()) == {0, 1}
        assert all((mon.group[i] == 0) == (p.ndim > 1) for i, p in enumerate(opt.flat.params))
        with pytest.raises(RuntimeError, match="attached already"):
            opt.attach_monitor()
        # a partial list of names, and none
        model2, opt2 = _build("plain")
        some = list(model2.named_parameters())[:2]
        mon2 = opt2.attach_monitor(names=some)
        assert mon2.names[:2] == [n for n, _ in some] and mon2.names[2:] == [f"param{i}" for i in range(2, len(opt2.flat.params))]
        assert mon2.read()["step"].size == 0 and mon2.nonfinite() == [] and "no record" in mon2.report()


def test_an_overflowed_fp16_step_names_its_tensor():
    """The second step's flat gradient gets one inf inside one tensor before step(): the record says skipped, no tensor moved,
    nonfinite() names that tensor and no other, and the next clean step records a finite, positive update."""
    d = _data()
    with ops.deterministic(), ops.compute_dtype(torch.float16):
        model, opt = _build("fp16_scaled")
        mon = opt.attach_monitor(names=model.named_parameters())
        victim = len(opt.flat.params) // 2
        at = opt.flat.offsets[victim] + opt.flat.params[victim].numel() // 2

        def step(poison):
            opt.zero_grad()
            out, _ = model(d.x)
            loss = U.compute_loss(_stack(out), d.y, d.mask, True)
            opt.scale_loss(loss).backward()
            if poison:
                opt.flat.flat_g[at] = float("inf")
            opt.step()

        step(False)
        assert mon.nonfinite() == []
        p = opt.flat.flat_p.clone()
        step(True)
        torch.cuda.synchronize()
        r = mon.read()
        assert r["step"].tolist() == [1, 2] and r["skipped"].tolist() == [False, True]
        assert _same_bits(opt.flat.flat_p, p) and not r["update_norm"][1].any() and (r["update_norm"][0] > 0).any()
        assert mon.nonfinite() == [(2, mon.names[victim], 1)] and mon.nonfinite(last=2) == [(2, mon.names[victim], 1)]
        assert np.isinf(r["global_grad_norm"][1]) and r["scale"][1] == 2.0 ** 14
        assert mon.names[victim] in mon.report() and "(skipped)" in mon.report()
        step(False)
        torch.cuda.synchronize()
        r = mon.read()
        assert r["skipped"].tolist() == [False, True, False] and r["scale"][2] == 2.0 ** 13             # the scale backed off
        assert np.isfinite(r["update_norm"][2]).all() and (r["update_norm"][2] > 0).any() and mon.nonfinite() == []
        assert mon.steps_seen() == 3 and mon.records_done() == 3 and opt.steps_done() == 2


# ---------------------------------------------------------------------------------------------
# C. reseed() and load_state_dict
# ---------------------------------------------------------------------------------------------
SHAPES = [(7, 3), (5,), (4, 2, 3, 3), (1,), (64,), (16, 8, 3, 3)]
STILL = 2                                          # the tensor whose gradient is zero: with no weight decay it does not move


def _tensor_optimiser(init):
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = U.FusedAdamW(ps, lr=1e-2, weight_decay=0.0, max_grad_norm=1.0)
    return ps, opt, opt.attach_monitor()


def _tensor_step(ps, opt, grads):
    opt.zero_grad()
    for i, (p, g) in enumerate(zip(ps, grads)):
        p.grad.copy_(torch.zeros_like(g) if i == STILL else g)
    opt.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize("how", ["nothing", "reseed", "load_state_dict"])
def test_a_restore_is_not_an_update(how):
    g = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [torch.randn(s, generator=g) for s in SHAPES]
    ps, opt, mon = _tensor_optimiser(init)
    sd = opt.state_dict()
    assert "monitor" not in sd["fused"]                                    # a diagnostic: not part of the state
    opt.flat.flat_p.add_(1.0)                                              # the weights change behind the optimiser's back: a restore
    if how == "reseed":
        mon.reseed()
    elif how == "load_state_dict":
        opt.load_state_dict(sd)
    _tensor_step(ps, opt, grads)
    r = mon.read()
    up, numel = r["update_norm"][0], r["numel"]
    assert r["names"] == [f"param{i}" for i in range(len(SHAPES))] and r["grad_zero_frac"][0, STILL] == 1.0
    if how == "nothing":
        # the restore shows up as one huge update, everywhere: every element moved by 1 less at most the step (lr = 0.01) and a rounding
        assert (up >= 0.98 * np.sqrt(numel)).all()
    else:
        moved = np.arange(len(SHAPES)) != STILL
        assert up[STILL] == 0.0 and (up[moved] > 0).all() and (up[moved] <= 0.011 * np.sqrt(numel[moved])).all()          # |step| <= lr per element
    assert "all-zero gradients: 1 tensors" in mon.report()


# ---------------------------------------------------------------------------------------------
# D. the captured step
# ---------------------------------------------------------------------------------------------
def graphed():
    """GraphedTrainStep with a monitor attached (every = 1, a ring of 4): counts after capture, a record per replay, each against
    the restatement on the static buffers.  Returns what the parent asserts on."""
    out = {}
    d = _data()
    with ops.deterministic():
        model = _model()
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, capturable=True)
        mon = opt.attach_monitor(every=1, history=4, names=model.named_parameters())
        g = U.GraphedTrainStep(model, opt, d.x, d.y, d.mask, True, warmup=2)
        torch.cuda.synchronize()
        out["after_capture"] = [mon.steps_seen(), mon.records_done(), opt.steps_done()]          # two eager warm-up steps; the capture ran nothing
        sizes = [q.numel() for q in opt.flat.params]
        bad_total, over_half, meta_ok = 0, 0, []
        for r in range(5):
            prev_h = mon.prev.cpu().numpy()
            g(d.x, d.y, d.mask)
            torch.cuda.synchronize()
            rows, sumsq, _ = _expected_record(opt, prev_h, (True, False))
            slot = (2 + r) % 4
            bad, half = M.compare_rows(mon.ring.cpu().numpy()[slot], rows, sizes)
            bad_total, over_half = bad_total + len(bad), over_half + half
            want_meta = np.array([3.0 + r, 1.0, sumsq, 0.0])
            meta_ok.append(bool(np.array_equal(_bits(mon.meta.cpu().numpy()[slot]), _bits(want_meta))))
            out.setdefault("counts", []).append([mon.records_done(), opt.steps_done()])
        out["mismatches"], out["over_half"], out["meta_ok"] = bad_total, over_half, meta_ok
        rd = mon.read()
        out["steps"] = rd["step"].tolist()
        out["moved"] = bool((rd["update_norm"] > 0).all(axis=0).any()) and bool(np.isfinite(rd["update_ratio"]).all())
        out["prev_is_p"] = bool(_same_bits(mon.prev, opt.flat.flat_p))
    return out


def test_graphed_step_records_on_every_replay():
    r = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[monitor] graphed step: {got}")
    assert got["after_capture"] == [2, 2, 2], got                 # the warm-up steps record, the capture itself runs nothing
    assert got["counts"] == [[k, k] for k in range(3, 8)], got    # records_done == steps_done after every replay
    assert got["steps"] == [4, 5, 6, 7], got                      # the ring holds the last `history` steps in order
    assert got["mismatches"] == 0 and all(got["meta_ok"]), got
    assert got["moved"] and got["prev_is_p"], got


if __name__ == "__main__":
    print(json.dumps(graphed()))
