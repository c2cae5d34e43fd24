"""The stream hand-off inventory and the schedules of tests/stream_order_cases.py, the part that needs no GPU.

1. Every (file, function) of the package that calls ``_on_side``, ``_schedule_join``, ``join_forward_side``, ``.wait_stream(``,
   ``.wait_event(``, ``.record_stream(``, ``torch.cuda.stream(`` or ``.record(`` has a row in the inventory, and every row still has
   its site: a hand-off added later without a row -- and so without a test -- fails here.
2. Every ``_on_side`` call outside ``prepack_begin`` passes a non-empty ``keep``.
3. Each schedule restores every attribute it patched, also when the body raises; its wrappers spin where they say, and ``plan_spin``
   meets the stated condition.
4. DESIGN.md "Stream hand-offs" holds the inventory's table.
No kernel is launched here."""
import ast
import os

import pytest

from conftest import ROOT

import stream_order_cases as SO

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops


# ---------------------------------------------------------------------------------------------
# 1, 2. the inventory against the sources
# ---------------------------------------------------------------------------------------------
def test_every_handoff_site_of_the_package_has_an_inventory_row():
    pairs, _ = SO.package_sites()
    rows = [(r.file, r.function) for r in SO.INVENTORY]
    assert len(rows) == len(set(rows)), "a site is listed twice"
    missing, gone = sorted(pairs - set(rows)), sorted(set(rows) - pairs)
    assert not missing, f"hand-off sites without a row in tests/stream_order_cases.py INVENTORY (and so without a test): {missing}"
    assert not gone, f"inventory rows whose site holds no hand-off any more: {gone}"
    # the files the step runs through are all there, and the walk found what a reader finds
    assert {f for f, _ in pairs} == {"ops.py", "ddp.py", "engine.py", "resnet.py", "modules.py"}
    for site in [("ops.py", "_on_side"), ("ops.py", "_schedule_join.join"), ("ops.py", "prepack_begin.pack_all"), ("ops.py", "_PackBatch.panel"),
                 ("ddp.py", "FlatDDP._launch"), ("engine.py", "GraphedTrainStep.__init__"), ("modules.py", "TemporalUNetDualView.forward")]:
        assert site in pairs, site


def test_every_row_names_tests_that_exist():
    with open(os.path.join(ROOT, "tests", SO.GPU_TEST_FILE)) as f:
        here = {n.name for n in ast.walk(ast.parse(f.read())) if isinstance(n, ast.FunctionDef)}
    for key, name in SO.TESTS.items():
        if "::" in name:
            path, fn = name.split("::")
            with open(os.path.join(ROOT, "tests", path)) as f:
                assert fn in {n.name for n in ast.walk(ast.parse(f.read())) if isinstance(n, ast.FunctionDef)}, name
        else:
            assert name in here, f"{key}: tests/{SO.GPU_TEST_FILE} has no {name}"
    used = set()
    for r in SO.INVENTORY:
        assert set(r.tests) <= set(SO.TESTS), (r.function, r.tests)
        # a row without a test orders nothing (timing events): it must say so
        assert r.tests or r.hazard.startswith("none"), f"{r.file} {r.function}: a hand-off with a hazard and no test"
        assert r.ordered_by and r.hazard and r.producer and r.consumer
        used |= set(r.tests)
    assert used == set(SO.TESTS), f"tests no row refers to: {sorted(set(SO.TESTS) - used)}"


def test_the_walk_sees_each_kind_of_call():
    src = ("import torch\n"
           "class A:\n"
           "    def f(self, s, e, t):\n"
           "        s.wait_stream(t)\n"
           "        def inner():\n"
           "            e.record(s)\n"
           "        with torch.cuda.stream(s):\n"
           "            t.record_stream(s)\n"
           "def g(d):\n"
           "    _on_side(d, lambda: None, keep=(d,))\n"
           "    ops.join_forward_side(d)\n"
           "    x.stream(d)\n"                      # not torch.cuda.stream
           "def h(m, e):\n"
           "    m.wait_event(e)\n"
           "_schedule_join(0)\n")
    got = sorted((fn, (c.func.attr if isinstance(c.func, ast.Attribute) else c.func.id)) for fn, c in SO.handoff_sites(src))
    assert got == sorted([("A.f", "wait_stream"), ("A.f.inner", "record"), ("A.f", "stream"), ("A.f", "record_stream"), ("g", "_on_side"),
                          ("g", "join_forward_side"), ("h", "wait_event"), ("<module>", "_schedule_join")])


def test_every_on_side_call_outside_prepack_begin_keeps_what_it_reads():
    _, on_side = SO.package_sites()
    assert len(on_side) >= 4
    seen_exempt = False
    for name, fn, call in on_side:
        keep = SO.keep_argument(call)
        if (name, fn) == ("ops.py", "prepack_begin"):
            seen_exempt = True          # its panels are allocated under the side stream and record_stream the main one themselves
            continue
        where = f"{name} {fn} line {call.lineno}"
        assert keep is not None, f"{where}: _on_side without keep: the buffers it reads are not protected from the caching allocator"
        if isinstance(keep, (ast.Tuple, ast.List)):
            assert len(keep.elts) >= 1, f"{where}: empty keep"
        else:
            assert not (isinstance(keep, ast.Constant) and not keep.value), f"{where}: empty keep"
    assert seen_exempt


# ---------------------------------------------------------------------------------------------
# 3. the schedules
# ---------------------------------------------------------------------------------------------
class Boom(Exception):
    pass


class FakeStream:
    cuda_stream = 0


class FakeOptimizer:
    steps = 0

    def step(self):
        self.steps += 1
        return "stepped"


@pytest.fixture
def spins(monkeypatch):
    """``L.lib.uclstm_stream_spin`` stubbed: the (microseconds) of every call."""
    calls = []

    def stub(us, stream):
        calls.append(int(us))
        return 0
    monkeypatch.setattr(L.lib, "uclstm_stream_spin", stub)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    return calls


def patched_state():
    return (ops._on_side, ops._PackBatch.__dict__["launch"], ops.prepack_begin, U.FusedAdamW.__dict__.get("step"),
            FakeOptimizer.__dict__["step"], (dict(ops._SIDE_STREAMS), dict(ops._LAUNCH_STREAMS)))


def contexts():
    spin = SO.Spin(7, 3)
    return {
        "one_stream": lambda: SO.one_stream(ops, "cuda:0", FakeStream()),
        "slow_side": lambda: SO.slow_side(ops, L, spin),
        "slow_main": lambda: SO.slow_main(ops, L, U.FusedAdamW, spin),
        "slow_main(other optimiser)": lambda: SO.slow_main(ops, L, FakeOptimizer, spin),
        "both": lambda: SO.both(ops, L, U.FusedAdamW, spin, spin),
    }


@pytest.mark.parametrize("raises", [False, True], ids=["returns", "raises"])
@pytest.mark.parametrize("name", list(contexts()))
def test_schedules_restore_everything_they_patched(name, raises, spins):
    before = patched_state()
    try:
        with contexts()[name]():
            assert patched_state() != before, f"{name} patched nothing"
            if raises:
                raise Boom()
    except Boom:
        assert raises
    after = patched_state()
    assert all(a is b for a, b in zip(after[:-1], before[:-1])) and after[-1] == before[-1], f"{name} left a patch behind"
    assert set(SO.SCHEDULES) <= {n.split("(")[0] for n in contexts()}
    assert not spins          # entering and leaving launches nothing


def test_one_stream_removes_the_key_it_added_and_restores_the_one_it_replaced(spins):
    s0, s1 = FakeStream(), FakeStream()
    key = "cuda:7"
    assert key not in ops._SIDE_STREAMS
    with SO.one_stream(ops, key, s0):
        assert ops._SIDE_STREAMS[key] is s0
        with SO.one_stream(ops, key, s1):
            assert ops._SIDE_STREAMS[key] is s1
        assert ops._SIDE_STREAMS[key] is s0
    assert key not in ops._SIDE_STREAMS


def test_one_stream_forgets_a_launch_stream_picked_inside_it(spins, monkeypatch):
    """ops.launch_stream caches its pick; inside one_stream it would be probed against [main, main]."""
    kept, inside = FakeStream(), FakeStream()
    monkeypatch.setitem(ops._LAUNCH_STREAMS, "cuda:6", kept)
    assert "cuda:7" not in ops._LAUNCH_STREAMS
    with SO.one_stream(ops, "cuda:7", FakeStream()):
        assert ops._LAUNCH_STREAMS["cuda:6"] is kept          # one probed against the real side stream stays in use
        ops._LAUNCH_STREAMS["cuda:7"] = inside
    assert "cuda:7" not in ops._LAUNCH_STREAMS and ops._LAUNCH_STREAMS["cuda:6"] is kept


def test_the_wrappers_spin_in_front_of_the_call(spins, monkeypatch):
    order = []
    monkeypatch.setattr(ops, "_on_side", lambda device, launch, keep=(): (order.append(("on_side", tuple(keep))), launch()))
    monkeypatch.setattr(ops._PackBatch, "launch", lambda self, side: order.append(("batch", side)))
    monkeypatch.setattr(ops, "prepack_begin", lambda: order.append(("begin",)))
    spin = SO.Spin(5, 2)
    with SO.slow_side(ops, L, spin) as side, SO.slow_main(ops, L, FakeOptimizer, spin) as main:
        def running_stats():
            order.append(("launch", len(spins)))
        ops._on_side("cuda:0", running_stats, ("t",))
        assert order == [("on_side", ("t",)), ("launch", 2)] and spins == [5, 5]          # the spins are inside, in front of launch
        stream = FakeStream()
        ops._PackBatch.launch(object(), stream)
        assert order[-1] == ("batch", stream) and spins == [5] * 4
        opt = FakeOptimizer()
        assert opt.step() == "stepped" and opt.steps == 1 and spins == [5] * 6
        ops.prepack_begin()
        assert order[-1] == ("begin",) and spins == [5] * 8
    assert (side.handoffs, side.injected_us, side.by_name) == (2, 20, {"running_stats": 1, "_PackBatch.launch": 1})
    assert (main.handoffs, main.injected_us, main.by_name) == (2, 20, {"step": 1, "prepack_begin": 1})
    assert side.captured == main.captured == 0
    # zero microseconds: hand-offs are counted, nothing is launched
    del spins[:]
    with SO.slow_main(ops, L, FakeOptimizer) as count:
        FakeOptimizer().step()
    assert count.handoffs == 1 and count.injected_us == 0 and not spins


@pytest.mark.parametrize("step_us,handoffs", [(1.0, 1), (180.0, 3), (400.0, 2), (3999.0, 2), (4001.0, 2), (45000.0, 2), (45000.0, 61), (250000.0, 7)])
def test_plan_spin_injects_at_least_twice_the_step_in_kernels_of_at_most_2000_us(step_us, handoffs):
    s = SO.plan_spin(step_us, handoffs)
    assert 1 <= s.us <= SO.MAX_SPIN_US == 2000 and s.reps >= 1
    assert s.per_handoff_us * handoffs >= 2.0 * step_us
    assert (s.per_handoff_us - s.reps) * handoffs < 2.0 * step_us + handoffs          # and no more than the rounding asks for
    assert s.reps == 1 or s.us > SO.MAX_SPIN_US // 2


def test_plan_spin_refuses_a_run_without_handoffs():
    with pytest.raises(ValueError):
        SO.plan_spin(100.0, 0)


# ---------------------------------------------------------------------------------------------
# 4. DESIGN.md
# ---------------------------------------------------------------------------------------------
def test_design_md_holds_the_inventory_table():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert "Stream hand-offs" in text
    start = text.index("Stream hand-offs")
    missing = [line for line in SO.design_table().splitlines() if line not in text[start:]]
    assert not missing, "DESIGN.md \"Stream hand-offs\" lacks these rows of stream_order_cases.design_table():\n" + "\n".join(missing)
