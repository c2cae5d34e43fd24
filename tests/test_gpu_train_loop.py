"""Several training steps in a row on the GPU: the host state that survives from one step to the next.

From step 1 on every forward and input-gradient panel of ``engine.train_step`` comes from a replay of the PREVIOUS step's pack
calls (``ops.prepack_begin`` / ``pack_weights``: ``_PACK_PLAN``, ``_PACK_READY``, the persistent ``_PackBatch``), keyed by the weight's
address, while ``FusedAdamW`` rewrites the weights through raw pointers.  A model trained on panels that are one step old still
learns, so nothing that compares the HIP path with itself, or watches the loss fall, notices.  Here:

1. look-ahead (batched), look-ahead panel by panel and in-line packing give the SAME four-step training run, bit for bit;
2. every look-ahead panel handed out in steps 1 to 3 equals the in-line pack of the live weight, bit for bit;
3. the same A/B through the events that change the plan between steps: an evaluation forward, a freeze, an unfreeze, an
   exception in the middle of the forward pass;
4. two models trained alternately in one process each follow the trajectory they follow alone;
5. a captured step owns the batch it captured: it survives the replacement of ``ops._PACK_BATCH`` and equals four eager steps
   (in a child process of its own, see tests/test_gpu_deterministic.py on captured graphs per process);
6. every step against the CPU oracle started from the device's own weights, with the stale-weights forward as the negative
   control (tests/test_train_loop_host.py shows on the CPU that the control has power).

Everything bit-exact runs in deterministic mode and asserts its yardstick first: two default runs are identical.  Measured figures
are printed (run with -s) and recorded in profiles/train_loop_parity.txt.
"""
import ctypes as C
import functools
import weakref

import pytest
import torch

import resnet_cases as RC
import train_loop_cases as TL
from conftest import load_golden, sub

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import ops
    from unet_convlstm_amd.engine import _stack
from oracle import unet_oracle as O

DEV = "cuda"
torch.set_num_threads(8)
SMALL = dict(base=8, B=1, T=2, hw=32)              # tests/test_gpu_deterministic.py's SMALL: the second, different model
WIDE = dict(base=64, B=1, T=2, hw=32)              # packing depends on channel counts, not on pixels: base 64 reaches all four pack families
RESNET = (2, 2, 64, 64, 1)                         # the smallest case of tests/test_gpu_resnet_unfrozen.py (B, T, H, W, LSTM layers)
RESNET_STAGES = ("layer3", "layer4")               # stem, layer1, layer2 stay frozen (their panels are in the plan too); layer4's strided
                                                   # block needs the lookahead=False temporary of resnet.s2_dgrad_weight
DTYPES = ["bf16", "fp16"]


def act(dtype):
    return torch.float16 if dtype == "fp16" else torch.bfloat16


@pytest.fixture(autouse=True)
def restore_switches():
    saved = (ops.PREPACK, ops.PACK_BATCHED, ops.is_deterministic(), ops.get_compute_dtype())
    fresh_plan()
    try:
        yield
    finally:
        ops.PREPACK, ops.PACK_BATCHED = saved[:2]
        ops.set_deterministic(saved[2])
        ops.set_compute_dtype(saved[3])
        ops.prepack_end()
        ops._PACK_PLAN.clear()


@pytest.fixture(scope="module", autouse=True)
def release_models():
    """The shared models, their initial states and the pinned comparison buffers go when the module is done."""
    yield
    _built.cache_clear()
    TL._STAGING[:] = [None, None]
    torch.cuda.empty_cache()


def fresh_plan():
    """What a new process starts with, except the batch object itself: it stays, as it would behind a second model."""
    ops.prepack_end()
    ops._PACK_PLAN.clear()


# ---------------------------------------------------------------------------------------------
# the models: built once per process, every run starts from the same restored state with a new optimiser
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _built(kind):
    if kind == "resnet":
        B, T, H, W, layers = RESNET
        model = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=layers).to(DEV)
        model.load_state_dict(RC.make_state(100 + layers, 1, layers), strict=True)
        model.unfreeze_encoder(RESNET_STAGES).train()
        batch = tuple(t.to(DEV) for t in RC.make_batch(200 + H + W, B, T, H, W))
    else:
        cfg = WIDE if kind == "wide" else SMALL
        torch.manual_seed(5)
        model = U.TemporalUNetDualView(1, 1, base_ch=cfg["base"], use_skip_lstm=True).to(DEV).train()
        d = U.SyntheticSequences(cfg["B"], cfg["T"], cfg["hw"], cfg["hw"], seed=6, kind="uniform")
        batch = (d.x, d.y, d.mask)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model, state, batch


def fresh(kind, dtype="bf16", **opt_kw):
    """(model, optimiser, batch, (names, sizes)) at the seeded initial state."""
    model, state, batch = _built(kind)
    model.load_state_dict(state)
    model.train()
    if dtype == "fp16":
        opt_kw = dict(loss_scale=2.0 ** 14, **opt_kw)
    opt = U.FusedAdamW(model.parameters(), lr=TL.LR, weight_decay=TL.WD, max_grad_norm=TL.CLIP, **opt_kw)
    return model, opt, batch, TL.layout(model)


def plan_keys():
    return {it[0] for it in ops._PACK_PLAN}


def train_run(kind, dtype, steps=TL.STEPS, spy=None, against=None, what=""):
    """``steps`` train_steps from the seeded state.  Returns the snapshots (or compares each with ``against`` and keeps none) and
    the number of distinct keys of the plan each step recorded."""
    fresh_plan()
    model, opt, (x, y, mask), (names, sizes) = fresh(kind, dtype)
    snaps, keys = [], []
    for k in range(steps):
        if spy is not None:
            spy.step = k
        loss, _ = U.train_step(model, opt, x, y, mask, True)
        torch.cuda.synchronize()
        keys.append(len(plan_keys()))
        s = TL.snapshot(model, opt, loss)
        if against is not None:
            TL.compare(f"{what} step {k}", against[k], s, names, sizes)
        else:
            snaps.append(s)
    return snaps, keys


# ---------------------------------------------------------------------------------------------
# 1. three ways of packing, one training run
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["wide", "resnet"])
def test_look_ahead_and_inline_packing_give_the_same_training_run(kind, dtype, monkeypatch):
    spy = TL.PackSpy(ops)
    monkeypatch.setattr(ops, "pack_weights", spy)
    with ops.deterministic(), ops.compute_dtype(act(dtype)):
        ref, keys = train_run(kind, dtype, spy=spy)
        default_calls, spy.calls = spy.calls, []
        # the yardstick first: two default runs are bit-identical
        train_run(kind, dtype, against=ref, what=f"{kind} {dtype}: second default run")
        for k in range(TL.STEPS):
            assert bool(torch.isfinite(ref[k]["loss"])), (k, ref[k]["loss"])
            if k:
                assert not TL.bits_equal(ref[k]["flat_p"], ref[k - 1]["flat_p"]), f"step {k} did not move the parameters"
        # power: from step 1 on the default run took every look-ahead panel from the replayed plan
        spy.calls = default_calls
        per_step = [(spy.hits(k), len(spy.of_step(k)), len(spy.misses(k))) for k in range(TL.STEPS)]
        print(f"[train loop] {kind} {dtype} default: (look-ahead hits, pack calls, in-line packs of look-ahead calls) per step {per_step}, "
              f"distinct keys in the plan {keys}")
        assert per_step[0][0] == 0 and per_step[0][1] > 0
        for k in range(1, TL.STEPS):
            assert not spy.misses(k), f"step {k}: {len(spy.misses(k))} look-ahead calls were packed in line"
            assert per_step[k][0] >= keys[k] > 0 and keys[k] == keys[0]
        if kind == "resnet":
            assert any(not c[1] for c in spy.calls), "the case has no lookahead=False temporary"
        spy.calls = []
        ops.PACK_BATCHED = False
        train_run(kind, dtype, spy=spy, against=ref, what=f"{kind} {dtype}: panel-by-panel look-ahead")
        single = [spy.hits(k) for k in range(TL.STEPS)]
        assert single[0] == 0 and all(h >= keys[k] for k, h in enumerate(single) if k), single
        spy.calls = []
        ops.PACK_BATCHED, ops.PREPACK = True, False
        train_run(kind, dtype, spy=spy, against=ref, what=f"{kind} {dtype}: in-line packing")
        assert spy.hits() == 0 and len(spy.calls) == sum(n for _, n, _ in per_step)
        print(f"[train loop] {kind} {dtype}: panel-by-panel look-ahead hits per step {single}; in-line run: 0 hits in {len(spy.calls)} calls; "
              f"{TL.STEPS} steps bit-identical three ways")


# ---------------------------------------------------------------------------------------------
# 2. the panels themselves
# ---------------------------------------------------------------------------------------------
def inline_pack(desc, w, off, dtype):
    wp = torch.empty((desc.N, desc.Ktot), dtype=dtype, device=w.device)
    L.check(L.kernels(dtype).uclstm_pack_weights(C.byref(desc), C.c_void_p(w.data_ptr() + 4 * off), C.c_void_p(wp.data_ptr()), ops._stream()),
            "pack_weights")
    return wp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["wide", "resnet"])
def test_every_look_ahead_panel_is_the_pack_of_the_live_weight(kind, dtype, monkeypatch):
    """train_step's own sequence written out (as tools/phase_times.py does), so that the panels can be looked at after the
    backward pass and before the optimiser changes the weights."""
    spy = TL.PackSpy(ops, keep_panels=True)
    monkeypatch.setattr(ops, "pack_weights", spy)
    counts = []
    with ops.compute_dtype(act(dtype)):
        model, opt, (x, y, mask), _ = fresh(kind, dtype)
        for k in range(TL.STEPS):
            spy.step, spy.panels = k, []
            opt.zero_grad(set_to_none=True)
            ops.prepack_begin()
            try:
                out, _ = model(x)
                loss = U.compute_loss(_stack(out), y, mask, True)
                opt.scale_loss(loss).backward()
            finally:
                ops.prepack_end()
            torch.cuda.synchronize()
            seen = {}
            for step, desc, w, off, dt, panel in spy.panels:
                seen.setdefault((w.data_ptr(), off, bytes(desc), dt), (desc, w, off, dt, panel))
            for desc, w, off, dt, panel in seen.values():
                want = inline_pack(desc, w, off, dt)
                assert panel.shape == want.shape and panel.dtype == want.dtype == act(dtype)
                assert torch.equal(panel.view(torch.int16), want.view(torch.int16)), \
                    f"{kind} {dtype} step {k}: the look-ahead panel of a [{tuple(w.shape)}] weight at offset {off} (N {desc.N}, K {desc.Ktot}) " \
                    f"differs from the pack of the live weight in {int((panel != want).sum())} elements"
            counts.append((len(seen), len(spy.panels)))
            assert bool(torch.isfinite(loss))
            opt.max_grad_norm = TL.CLIP
            opt.step()
    print(f"[train loop] {kind} {dtype}: (distinct look-ahead panels compared with the in-line pack, hits) per step {counts}")
    assert counts[0] == (0, 0) and all(n > 0 and n == counts[1][0] for n, _ in counts[1:])


# ---------------------------------------------------------------------------------------------
# 3. the plan changes between steps
# ---------------------------------------------------------------------------------------------
ENCODER = ("inc", "down1", "down2", "down3", "bottleneck")


def stop_after(module):
    """What a raising forward hook does -- run the module's forward, then raise a plain RuntimeError on the host -- put where the
    model really calls ``up1``: it goes through ``forward_nhwc``, not ``__call__``, so a registered forward hook would never fire
    (and the event would test nothing).  Returns the function that removes it."""
    real = module.forward_nhwc

    def forward_nhwc(*args, **kw):
        real(*args, **kw)
        raise RuntimeError("stop inside the forward pass")
    module.forward_nhwc = forward_nhwc
    return lambda: delattr(module, "forward_nhwc")


def event_run(prepack, against=None):
    """The events of test 3 on the base-64 model; a snapshot after every event.  Returns (snapshots, notes)."""
    fresh_plan()
    ops.PREPACK = prepack
    model, opt, (x, y, mask), (names, sizes) = fresh("wide")
    snaps, notes, last = [], {}, [None]

    def done(what, **extra):
        torch.cuda.synchronize()
        s = TL.snapshot(model, opt, last[0], **extra)
        if against is not None:
            TL.compare(f"event {len(snaps)} ({what})", against[len(snaps)], s, names, sizes)
        snaps.append(s if against is None else None)

    def step(what):
        last[0], _ = U.train_step(model, opt, x, y, mask, True)
        done(what)

    def freeze(mods, on):
        for name in mods:
            for p in getattr(model, name).parameters():
                p.requires_grad_(not on)

    try:
        step("step")
        step("step")
        model.eval()
        with torch.no_grad():
            out, _ = model(x)
        y_eval = _stack(out).clone()
        model.train()
        done("evaluation forward", y_eval=y_eval)
        step("step after the evaluation")
        before = (ops._PACK_BATCH, None if ops._PACK_BATCH is None else ops._PACK_BATCH.sig, plan_keys())
        freeze(("temporal",), True)                       # the gate weights lose their gradient; the input still needs one
        step("temporal ConvLSTM frozen")
        step("temporal ConvLSTM frozen, second step")
        notes["temporal_only_changed_plan"] = plan_keys() != before[2]
        freeze(ENCODER, True)                             # ... now it does not: the ConvLSTMs' x halves and every encoder input gradient leave the plan
        step("encoder and temporal ConvLSTM frozen")
        step("encoder and temporal ConvLSTM frozen, second step")
        notes["freeze_changed_plan"] = plan_keys() != before[2]
        notes["batch_rebuilt"] = prepack and (ops._PACK_BATCH is not before[0] and ops._PACK_BATCH.sig != before[1])
        notes["keys"] = (len(before[2]), len(plan_keys()))
        freeze(ENCODER + ("temporal",), False)
        step("unfrozen")
        remove = stop_after(model.up1)
        try:
            with pytest.raises(RuntimeError, match="stop inside the forward pass"):
                U.train_step(model, opt, x, y, mask, True)
        finally:
            remove()
        assert "forward_nhwc" not in vars(model.up1)
        notes["clean_after_exception"] = (len(ops._PACK_READY), bool(ops._PACK_RECORDING))
        notes["partial_plan"] = len(plan_keys())
        step("step after the exception")
        step("second step after the exception")
        notes["clean_at_end"] = (len(ops._PACK_READY), bool(ops._PACK_RECORDING))
        notes["final_plan"] = len(plan_keys())
    finally:
        freeze(ENCODER + ("temporal",), False)
    return snaps, notes


def test_the_plan_changes_between_steps():
    """The first freeze -- ``requires_grad_(False)`` on the temporal ConvLSTM's weights -- does not change the plan on its own: a
    frozen gate weight drops its weight-gradient GEMM, which packs nothing, while the input gradient and hence both input-gradient
    panels stay (``notes["temporal_only_changed_plan"]`` is printed).  So that the event has the power asked for, the freeze goes
    on to the encoder, after which the ConvLSTMs' input halves and every encoder input-gradient panel leave the plan; the change of
    the signature and the rebuilt batch are asserted on that."""
    with ops.deterministic():
        ref, n_ref = event_run(False)
        _, n = event_run(True, against=ref)
    print(f"[train loop] plan events, base 64: {len(ref)} events bit-identical, look-ahead against in-line; plan keys before / after the freeze "
          f"{n['keys']}, temporal-only freeze changed the plan: {n['temporal_only_changed_plan']}, batch rebuilt: {n['batch_rebuilt']}, plan after "
          f"the exception {n['partial_plan']} keys, at the end {n['final_plan']}")
    assert len(ref) == 11
    assert n["freeze_changed_plan"] and n["batch_rebuilt"], n
    assert n["clean_after_exception"] == (0, False) and n["clean_at_end"] == (0, False), n
    assert n_ref["clean_after_exception"] == (0, False)
    assert 0 < n["partial_plan"] < n["final_plan"] == n["keys"][0]
    assert not TL.bits_equal(ref[3]["flat_p"], ref[1]["flat_p"]) and TL.bits_equal(ref[2]["flat_p"], ref[1]["flat_p"])


# ---------------------------------------------------------------------------------------------
# 4. two models in one process
# ---------------------------------------------------------------------------------------------
def test_two_models_trained_alternately_follow_their_own_trajectories():
    with ops.deterministic():
        alone = {kind: train_run(kind, "bf16", steps=3)[0] for kind in ("wide", "small")}
        fresh_plan()
        runs = {kind: fresh(kind) for kind in ("wide", "small")}
        for k in range(3):
            for kind in ("wide", "small"):
                model, opt, (x, y, mask), (names, sizes) = runs[kind]
                loss, _ = U.train_step(model, opt, x, y, mask, True)
                torch.cuda.synchronize()
                TL.compare(f"{kind} model, step {k} of the alternating run against the run alone", alone[kind][k], TL.snapshot(model, opt, loss), names, sizes)
    for kind in alone:
        assert not TL.bits_equal(alone[kind][2]["flat_p"], alone[kind][1]["flat_p"])
    print("[train loop] base-64 and base-8 models trained alternately (A, B, A, B, A, B): each bit-identical to its run alone")


# ---------------------------------------------------------------------------------------------
# 5. a captured step owns its batch (child process)
# ---------------------------------------------------------------------------------------------
def graph_child():
    """Runs in a process of its own.  Returns what the parent asserts on; stops before the first replay if the captured batch
    is not provably alive."""
    out = dict(checks=[], steps=[], other_model=None)
    ops.set_deterministic(True)

    def make(cfg, capturable):
        torch.manual_seed(5)
        m = U.TemporalUNetDualView(1, 1, base_ch=cfg["base"], use_skip_lstm=True).to(DEV).train()
        o = U.FusedAdamW(m.parameters(), lr=TL.LR, weight_decay=TL.WD, max_grad_norm=TL.CLIP, capturable=capturable)
        return m, o

    d = U.SyntheticSequences(SMALL["B"], SMALL["T"], SMALL["hw"], SMALL["hw"], seed=6, kind="uniform")
    m8, o8 = make(SMALL, True)
    for _ in range(2):                                     # on the default stream: the batch lives in the default pool
        U.train_step(m8, o8, d.x, d.y, d.mask, True)
    eager_batch = ops._PACK_BATCH
    g = U.GraphedTrainStep(m8, o8, d.x, d.y, d.mask, True, warmup=2)
    captured = ops._PACK_BATCH
    alive = weakref.ref(captured)
    ptrs = sorted(wp.data_ptr() for wp, _ in captured.panels.values()) + [captured.table.data_ptr()]
    out["checks"].append(("the graph holds the batch its capture used", getattr(g, "_pack_batch", None) is captured))
    out["checks"].append(("the captured batch is the eager steps' (allocated on the default stream)", captured is eager_batch and captured is not None))
    del captured, eager_batch
    m64, o64 = make(WIDE, False)
    for _ in range(2):
        U.train_step(m64, o64, d.x, d.y, d.mask, True)
    torch.cuda.synchronize()
    live = alive()
    out["checks"].append(("ops._PACK_BATCH was replaced", ops._PACK_BATCH is not None and ops._PACK_BATCH is not live))
    out["checks"].append(("the captured batch is alive", live is not None))
    out["checks"].append(("its panels and job table did not move",
                          live is not None and sorted(wp.data_ptr() for wp, _ in live.panels.values()) + [live.table.data_ptr()] == ptrs))
    del live
    out["panels"] = len(ptrs) - 1
    if not all(ok for _, ok in out["checks"]):
        return out                                         # no replay of a graph whose memory may be gone
    twin, otwin = make(SMALL, True)
    twin.load_state_dict(m8.state_dict())
    otwin.m.copy_(o8.m)
    otwin.v.copy_(o8.v)
    otwin.hyper.copy_(o8.hyper)
    names, sizes = TL.layout(m8)
    other = TL.snapshot(m64, o64, torch.zeros(()))
    p_start = o8.flat.flat_p.clone()
    for k in range(4):
        lg, _ = g(d.x, d.y, d.mask)
        le, _ = U.train_step(twin, otwin, d.x, d.y, d.mask, True)
        torch.cuda.synchronize()
        a = TL.snapshot(m8, o8, lg, step_count=o8.hyper[6:7])
        b = TL.snapshot(twin, otwin, le, step_count=otwin.hyper[6:7])
        diff = TL.first_difference(a, b, names, sizes)
        out["steps"].append(dict(diff=diff, loss=float(lg), count=int(o8.hyper[6]), finite=bool(torch.isfinite(lg))))
    diff = TL.first_difference(other, TL.snapshot(m64, o64, torch.zeros(())), *TL.layout(m64))
    out["other_model"] = diff
    out["moved"] = not TL.bits_equal(o8.flat.flat_p, p_start)
    return out


def test_a_captured_step_owns_its_batch_and_equals_four_eager_steps():
    """The lifetime is checked on the host BEFORE anything is replayed: a graph whose panels were freed would write freed memory.
    Then four replays against four eager steps of a twin from the same state, the several-steps comparison that
    tests/test_gpu_host_semantics.py::test_graphed_train_step_replays_the_eager_step leaves out (it predates deterministic mode)."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[train loop] graph child: {got}")
    for what, ok in got["checks"]:
        assert ok, f"not true before the first replay: {what}"
    assert len(got["checks"]) == 5 and got["panels"] > 0 and len(got["steps"]) == 4
    counts = [s["count"] for s in got["steps"]]
    assert counts == [5, 6, 7, 8], counts                  # 2 eager + 2 warm-up steps, then one per replay
    for k, s in enumerate(got["steps"]):
        assert s["finite"] and s["diff"] is None, f"replay {k} differs from the eager twin's step: first differing tensor {s['diff']}"
    assert got["moved"] and len({s["loss"] for s in got["steps"]}) == 4
    assert got["other_model"] is None, f"the replays changed the other model: {got['other_model']}"


# ---------------------------------------------------------------------------------------------
# 6. each step against the oracle, from the device's own state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["model_noskip", "model_skip"])
def test_each_step_against_the_oracle_from_the_devices_own_state(name):
    """Bounds: the ones the project holds for step 0 (tests/test_gpu_model.py: per-timestep rel-L2 <= 1.5e-2, loss within 2e-3),
    at every step.  Negative control without further GPU work: the same y_pred of steps 2 and 3 against the oracle on the PREVIOUS
    snapshot must be at least 4 x the bound away."""
    g = load_golden(name)
    p = sub(g, "p/")
    model = U.TemporalUNetDualView(1, 1, base_ch=p["inc.net.0.weight"].shape[0], lstm_layers=1,
                                   use_skip_lstm="lstm_skip3.layers.0.conv.weight" in p).to(DEV)
    res = model.load_state_dict(p, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.train()
    opt = U.FusedAdamW(model.parameters(), lr=TL.LR, weight_decay=TL.WD, max_grad_norm=TL.CLIP)
    x, y, mask = g["x"], g["y"], g["mask"]
    xd, yd, md = x.to(DEV), y.to(DEV), mask.to(DEV)
    T = x.shape[1]
    got, refs, rows = [], [], []
    for k in range(1, TL.ORACLE_STEPS + 1):
        sd = {key: v.detach().cpu().clone() for key, v in model.state_dict().items()}
        loss, y_pred = U.train_step(model, opt, xd, yd, md, True)
        with torch.no_grad(), O.bf16_storage():
            outs, _ = O.model_forward(sd, x, None, True, {})
        ref = torch.stack(outs, 1)
        ref_loss = float(O.compute_loss(ref, y, mask, True))
        got.append(y_pred.cpu())
        refs.append(ref)
        errs = TL.per_t(got[-1], ref)
        e_loss = abs(float(loss) - ref_loss) / abs(ref_loss)
        rows.append((errs, e_loss))
        print(f"[train loop] {name} step {k}: per-timestep rel-L2 vs the bf16-storage oracle on the device's own weights {[round(e, 5) for e in errs]} "
              f"(error / bound {max(errs) / TL.PER_T_BOUND:.3f}); loss {float(loss):.6f} vs {ref_loss:.6f} (error / bound {e_loss / TL.LOSS_BOUND:.3f})")
        assert opt.steps_done() == k
        for key, v in model.state_dict().items():
            if key.endswith("num_batches_tracked"):
                assert int(v) == k * T, (key, int(v))
    stale = TL.stale_distances(got, refs)
    for k, errs in zip(range(2, TL.ORACLE_STEPS + 1), stale):
        print(f"[train loop] {name} step {k}: the same y_pred vs the oracle on the PREVIOUS step's weights {[round(e, 4) for e in errs]} "
              f"(error / bound {min(errs) / TL.PER_T_BOUND:.1f}, required >= {TL.STALE_MIN / TL.PER_T_BOUND:.0f})")
    for k, (errs, e_loss) in enumerate(rows, start=1):
        assert max(errs) <= TL.PER_T_BOUND, f"{name} step {k}: per-timestep rel-L2 {errs} > {TL.PER_T_BOUND}"
        assert e_loss <= TL.LOSS_BOUND, f"{name} step {k}: loss off by {e_loss:.3e} > {TL.LOSS_BOUND}"
    for k, errs in zip(range(2, TL.ORACLE_STEPS + 1), stale):
        assert min(errs) >= TL.STALE_MIN, f"{name} step {k}: stale weights only {errs} away, the control has no power"


if __name__ == "__main__":
    import json
    print(json.dumps(graph_child()))
