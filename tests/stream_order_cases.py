"""The stream hand-offs of the package and the schedules that bend them (imports without a GPU).

A training step runs on up to three HIP streams: the main stream, the side stream of ``ops.side_stream``
(weight gradients, BatchNorm running statistics and parameter gradients, look-ahead panels) and ``FlatDDP``'s kernel-less launch
stream.  Every hand-off between them is correct only because somebody wrote a wait, an event or a ``record_stream``; at natural
timing the host enqueues so slowly that a missing one still gives the right bits.  This file holds

  * ``INVENTORY``: one row per (file, function) of the package that contains a hand-off, with what orders it and which test of
    tests/test_gpu_stream_order.py covers it (tests/test_stream_order_host.py walks the sources and fails on a site without a row);
  * the schedules, context managers that patch and restore: ``one_stream`` (the race-free reference: the side stream IS the
    current stream), ``slow_side`` and ``slow_main`` (``uclstm_stream_spin`` in front of every hand-off on that stream) and ``both``;
  * ``plan_spin``: the spin per hand-off from the measured device time of the undelayed step;
  * ``design_table``: the inventory as the markdown table of DESIGN.md "Stream hand-offs".
"""
import ast
import contextlib
import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Tuple
from unittest import mock

PACKAGE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unet-convlstm_amd")
GPU_TEST_FILE = "test_gpu_stream_order.py"
MAX_SPIN_US = 2000          # no single spin kernel runs longer
MIN_TOTAL_FACTOR = 2.0      # total injected on the delayed stream >= this x the undelayed step's device time

# the tests of tests/test_gpu_stream_order.py, by the letter the rows below use
TESTS = {
    "A": "test_operator_gradients_under_a_delayed_side_stream",
    "A'": "test_operator_gradients_under_a_delayed_side_stream_and_reallocation",
    "B": "test_three_steps_under_every_schedule",
    "C": "test_a_step_captured_under_a_delayed_side_stream_equals_eager_one_stream_steps",
    "D": "test_flat_ddp_buckets_wait_for_the_delayed_side_stream",
    "E": "test_control_without_the_join_the_delayed_gradient_is_seen_missing",
    "probe": "test_gpu_ops.py::test_side_stream_is_probed_to_run_concurrently_with_the_main_stream",
}


@dataclass(frozen=True)
class HandOff:
    file: str               # under unet-convlstm_amd/
    function: str           # dotted name of the innermost enclosing def (classes and outer functions included)
    producer: str           # stream whose work is handed over
    consumer: str           # stream that must not run ahead of it
    ordered_by: str         # the wait / event / engine callback / record_stream that orders them
    hazard: str             # what would be read stale, or overwritten early, without it
    tests: Tuple[str, ...]  # keys of TESTS


INVENTORY = [
    # ---- ops.py: the side stream itself
    HandOff("ops.py", "_on_side", "main", "side",
            "side.wait_stream(main) before launch(); record_stream(side) on every tensor of keep=",
            "the side launch reads its operands before the main stream wrote them; a kept operand freed by the main stream is "
            "recycled by the caching allocator under the side stream's read", ("A", "A'", "B")),
    HandOff("ops.py", "wgrad_into_param", "side", "main",
            "_on_side(keep=inputs) for the fork, _schedule_join for the join",
            "weight.grad read (clip, AdamW, bucket copy) before the GEMM and its unpack-accumulate ran; x / dz recycled under the GEMM",
            ("A", "A'", "B", "E")),
    HandOff("ops.py", "_schedule_join.join", "side", "main",
            "main.wait_stream(side) in the autograd-engine callback _schedule_join queues once per backward pass",
            "every gradient written on the side stream is read stale by whatever follows backward() (B: clip and AdamW read "
            "flat_g on the main stream with no synchronisation in between; A synchronises before it reads)", ("B", "E")),
    HandOff("ops.py", "_bn_forward_stats", "main", "side",
            "_on_side(keep=(stats,)); the join is join_forward_side via _FWD_SIDE_PENDING",
            "running statistics updated from partial sums the convolution has not written, or from a recycled stats buffer",
            ("A", "A'", "B")),
    HandOff("ops.py", "bn_param_grads", "side", "main", "_on_side(keep=(sums,)) for the fork, _schedule_join for the join",
            "gamma.grad / beta.grad read before the side kernel added the groups; sums recycled under it", ("A", "A'", "B")),
    HandOff("ops.py", "join_forward_side", "side", "main", "main.wait_stream(side) if a forward pass put work there",
            "evaluation-mode BatchNorm, state_dict() or a checkpoint reads running statistics one update old", ("A",)),
    HandOff("ops.py", "conv_bn_stats", "side", "main", "join_forward_side before an evaluation-statistics stage",
            "bn_finalize(eval) reads running statistics the side stream is still updating (operator train-then-eval)", ("A",)),
    HandOff("ops.py", "conv_bn_fold", "side", "main", "join_forward_side before _eval_bn_constants",
            "the folded scale / shift are computed from running statistics one update old (operator train-then-eval)", ("A",)),
    # ---- ops.py: look-ahead panels
    HandOff("ops.py", "prepack_begin", "main", "side",
            "side.wait_stream(main) before _PackBatch.launch; _on_side for the panel-by-panel route",
            "panels packed from the weights of the previous step (optimiser step not finished), or persistent panels overwritten "
            "under their last readers of the previous step", ("B", "C")),
    HandOff("ops.py", "prepack_begin.pack_all", "side", "main",
            "one event per panel recorded on side; wp.record_stream(main) on the panel allocated under the side stream",
            "a convolution reads a panel that is not packed yet; a dropped panel is recycled by side-stream allocations under its "
            "main-stream reader", ("B",)),
    HandOff("ops.py", "_PackBatch.launch", "side", "main", "events[s].record(side) behind segment s",
            "(produces the events _PackBatch.panel waits for)", ("B", "C")),
    HandOff("ops.py", "_PackBatch.panel", "side", "main", "main.wait_event(events[segment])",
            "a convolution multiplies a panel of the previous step, or a half-written one", ("B", "C")),
    HandOff("ops.py", "pack_weights", "side", "main", "main.wait_event(panel's event) on the panel-by-panel route",
            "as above, UCLSTM_PACK_BATCHED=0", ("B",)),
    # ---- ops.py: events that order nothing
    HandOff("ops.py", "_timed", "main", "main", "timing events on the launch stream (ops.PROFILE only)", "none: measures, orders nothing", ()),
    HandOff("ops.py", "_timed_hbm", "main", "main", "timing events on the launch stream (ops.PROFILE_HBM only)",
            "none: measures, orders nothing", ()),
    HandOff("ops.py", "_streams_overlap", "main", "candidate", "timing events around two spin kernels, both streams synchronised",
            "none: the probe that chooses the side stream; a wrong answer serialises, it does not race", ("probe",)),
    # ---- ddp.py
    HandOff("ddp.py", "FlatDDP._launch", "main + side", "launch -> RCCL",
            "launch.wait_stream(main), launch.wait_stream(side), launch.wait_stream(current); the copy and the collective under "
            "torch.cuda.stream(launch)",
            "a bucket staged or all-reduced before the side stream's accumulation: with bf16 staging finalize() copies the stale "
            "stage back over flat_g even at world size 1", ("D",)),
    # ---- engine.py
    HandOff("engine.py", "GraphedTrainStep.__init__", "current <-> warm-up", "warm-up <-> current",
            "s.wait_stream(current) before the eager warm-up steps, current.wait_stream(s) after them",
            "warm-up steps start from clones still being written; the capture starts before the warm-up finished (C executes both "
            "waits but nothing it compares would differ without them: executed, not discriminated)", ("C",)),
    # ---- resnet.py / modules.py: the joins at the public forwards
    HandOff("resnet.py", "PretrainedTemporalUNet.forward", "side", "main", "join_forward_side when forward returns",
            "running statistics of the trainable encoder and the decoder read one update old after forward() (operator "
            "resnet-forward: the buffers cloned on the main stream when forward returns)", ("A",)),
    HandOff("resnet.py", "PretrainedTemporalUNet.step_nhwc", "side", "main", "join_forward_side before the decoder",
            "none: the method raises in grad mode and while any BatchNorm uses batch statistics, and every evaluation-mode stage "
            "above it has joined already, so nothing can be pending there", ()),
    HandOff("modules.py", "DoubleConv.forward", "side", "main", "join_forward_side before the layout conversion",
            "running statistics read one update old after a stand-alone block's forward (operator doubleconv: the buffers "
            "cloned on the main stream when forward returns, before backward)", ("A",)),
    HandOff("modules.py", "Down.forward", "side", "main", "join_forward_side before the layout conversion",
            "as DoubleConv.forward (operator down)", ("A",)),
    HandOff("modules.py", "Up.forward", "side", "main", "join_forward_side before the layout conversion",
            "as DoubleConv.forward (operator up-two-sources)", ("A",)),
    HandOff("modules.py", "TemporalUNetDualView.encode_once", "side", "main", "join_forward_side before the layout conversions",
            "as DoubleConv.forward (operator encode-once)", ("A",)),
    HandOff("modules.py", "TemporalUNetDualView.forward", "side", "main", "join_forward_side in the finally of forward",
            "whatever reads the running statistics after a training-mode forward without a backward pass (validation with "
            "batch statistics, state_dict()) reads them one update old (operator unet-forward)", ("A",)),
    HandOff("modules.py", "TemporalUNetDualView.step_nhwc", "side", "main", "join_forward_side before the output convolution",
            "as DoubleConv.forward, frame by frame (operator unet-step-nhwc, training mode)", ("A",)),
]


# ---------------------------------------------------------------------------------------------
# the sources, walked with ast
# ---------------------------------------------------------------------------------------------
CALL_NAMES = ("_on_side", "_schedule_join", "join_forward_side")
METHOD_NAMES = ("wait_stream", "wait_event", "record_stream", "record")


def _is_handoff_call(node: ast.Call) -> bool:
    f = node.func
    if isinstance(f, ast.Name):
        return f.id in CALL_NAMES
    if isinstance(f, ast.Attribute):
        if f.attr in CALL_NAMES or f.attr in METHOD_NAMES:
            return True
        # torch.cuda.stream(...)
        return (f.attr == "stream" and isinstance(f.value, ast.Attribute) and f.value.attr == "cuda"
                and isinstance(f.value.value, ast.Name) and f.value.value.id == "torch")
    return False


def handoff_sites(source: str):
    """[(dotted name of the innermost enclosing def, call node)] of every hand-off call in ``source``."""
    out = []

    def walk(node, scope):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                walk(child, scope + [child.name])
            else:
                if isinstance(child, ast.Call) and _is_handoff_call(child):
                    out.append((".".join(scope) or "<module>", child))
                walk(child, scope)

    walk(ast.parse(source), [])
    return out


def package_sites(package_dir: str = PACKAGE_DIR):
    """{(file, function)} over every Python source of the package, and [(file, function, call node)] of the ``_on_side`` calls."""
    pairs, on_side = set(), []
    for name in sorted(os.listdir(package_dir)):
        if not name.endswith(".py"):
            continue
        with open(os.path.join(package_dir, name)) as f:
            for fn, call in handoff_sites(f.read()):
                pairs.add((name, fn))
                callee = call.func.id if isinstance(call.func, ast.Name) else call.func.attr
                if callee == "_on_side":
                    on_side.append((name, fn, call))
    return pairs, on_side


def keep_argument(call: ast.Call):
    """The ``keep`` argument of an ``_on_side(device, launch, keep)`` call as an ast node, or None when it is not passed."""
    if len(call.args) >= 3:
        return call.args[2]
    for kw in call.keywords:
        if kw.arg == "keep":
            return kw.value
    return None


def design_table() -> str:
    """The inventory as the markdown table of DESIGN.md "Stream hand-offs" (tests/test_stream_order_host.py holds the two equal)."""
    lines = ["| site | producer -> consumer | ordered by | without it | test |", "|---|---|---|---|---|"]
    for r in INVENTORY:
        tests = ", ".join(r.tests) if r.tests else "-"
        lines.append(f"| `{r.file}` `{r.function}` | {r.producer} -> {r.consumer} | {r.ordered_by} | {r.hazard} | {tests} |")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------
# spin length
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Spin:
    """``reps`` spin kernels of ``us`` microseconds in front of every hand-off (us 0: count the hand-offs, delay nothing)."""
    us: int = 0
    reps: int = 1

    @property
    def per_handoff_us(self) -> int:
        return self.us * self.reps


def plan_spin(step_us: float, handoffs: int) -> Spin:
    """The spin in front of each of ``handoffs`` hand-offs such that their sum is at least MIN_TOTAL_FACTOR x ``step_us`` (the
    device time of the undelayed step), cut into kernels of at most MAX_SPIN_US each."""
    if handoffs < 1:
        raise ValueError("plan_spin: the undelayed run made no hand-off on this stream, so there is nothing to delay")
    per = max(1, math.ceil(MIN_TOTAL_FACTOR * step_us / handoffs))
    reps = math.ceil(per / MAX_SPIN_US)
    return Spin(math.ceil(per / reps), reps)


# ---------------------------------------------------------------------------------------------
# schedules
# ---------------------------------------------------------------------------------------------
def _capturing() -> bool:
    import torch
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class Schedule(contextlib.ExitStack):
    """A context manager whose ``install()`` enters ``unittest.mock`` patches (``patch.object`` / ``patch.dict``) on itself: every
    one of them is undone on exit, also when the body raises.  ``handoffs``: wrapped calls seen so far (``by_name``: per wrapped
    function or launch closure; ``captured``: those made while the current stream was capturing a graph); ``injected_us``:
    microseconds of spin enqueued so far."""

    def __init__(self, name: str):
        super().__init__()
        self.name, self.handoffs, self.injected_us, self.captured = name, 0, 0, 0
        self.by_name: dict = {}

    def install(self) -> None:
        raise NotImplementedError

    def __enter__(self):
        super().__enter__()
        try:
            self.install()
        except BaseException:
            self.close()
            raise
        return self

    def _spin(self, lib_mod, spin: Spin, stream_ptr, what: str = "") -> None:
        self.handoffs += 1
        self.by_name[what] = self.by_name.get(what, 0) + 1
        if _capturing():
            self.captured += 1
        for _ in range(spin.reps if spin.us > 0 else 0):
            lib_mod.check(lib_mod.lib.uclstm_stream_spin(spin.us, stream_ptr), "stream_spin")
            self.injected_us += spin.us


class one_stream(Schedule):
    """``ops._SIDE_STREAMS[str(device)]`` is ``stream`` (default: the stream current on entry): every side launch runs in program
    order on that one stream with the same descriptors (``_WGRAD_OVERLAPPED`` is still set inside ``wgrad_into_param``, so pixel-range
    counts and summation order are those of the two-stream run).  Race-free by construction."""

    def __init__(self, ops, device, stream=None):
        super().__init__("one_stream")
        self.ops, self.device, self.stream = ops, device, stream

    def install(self):
        stream = self.stream
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device)
        self.enter_context(mock.patch.dict(self.ops._SIDE_STREAMS, {str(self.device): stream}))
        # a launch stream chosen in here would be probed against [main, main] and kept for the rest of the process
        # (ops.launch_stream caches its pick): whatever is cached on entry comes back on exit, a pick made inside is dropped
        self.enter_context(mock.patch.dict(self.ops._LAUNCH_STREAMS))


class slow_side(Schedule):
    """``ops._on_side``: ``launch`` is preceded by the spin on ``ops._stream()`` -- the side stream, which is current there;
    ``ops._PackBatch.launch`` spins on ``side`` first."""

    def __init__(self, ops, lib_mod, spin: Spin = Spin()):
        super().__init__("slow_side")
        self.ops, self.lib_mod, self.spin = ops, lib_mod, spin

    def install(self):
        ops, me = self.ops, self
        on_side, batch_launch = ops._on_side, ops._PackBatch.launch

        def delayed_on_side(device, launch, keep=()):
            def delayed():
                me._spin(me.lib_mod, me.spin, ops._stream(), getattr(launch, "__name__", "launch"))
                launch()
            return on_side(device, delayed, keep)

        def delayed_batch_launch(batch, side):
            me._spin(me.lib_mod, me.spin, C.c_void_p(side.cuda_stream), "_PackBatch.launch")
            return batch_launch(batch, side)

        self.enter_context(mock.patch.object(ops, "_on_side", delayed_on_side))
        self.enter_context(mock.patch.object(ops._PackBatch, "launch", delayed_batch_launch))


class slow_main(Schedule):
    """The optimiser's ``step`` and ``ops.prepack_begin`` spin on the current stream before they run: without the
    ``side.wait_stream(main)`` of ``prepack_begin`` the panels would be packed from the previous weights, or under their last readers."""

    def __init__(self, ops, lib_mod, optimizer_cls, spin: Spin = Spin()):
        super().__init__("slow_main")
        self.ops, self.lib_mod, self.optimizer_cls, self.spin = ops, lib_mod, optimizer_cls, spin

    def install(self):
        ops, me = self.ops, self
        step, begin = self.optimizer_cls.step, ops.prepack_begin

        def delayed_step(opt, *a, **k):
            me._spin(me.lib_mod, me.spin, ops._stream(), "step")
            return step(opt, *a, **k)

        def delayed_begin():
            me._spin(me.lib_mod, me.spin, ops._stream(), "prepack_begin")
            return begin()

        self.enter_context(mock.patch.object(self.optimizer_cls, "step", delayed_step))
        self.enter_context(mock.patch.object(ops, "prepack_begin", delayed_begin))


@contextlib.contextmanager
def both(ops, lib_mod, optimizer_cls, side_spin: Spin = Spin(), main_spin: Spin = Spin()):
    """``slow_side`` and ``slow_main`` together; yields the two schedules."""
    with slow_side(ops, lib_mod, side_spin) as s, slow_main(ops, lib_mod, optimizer_cls, main_spin) as m:
        yield s, m


SCHEDULES = ("one_stream", "slow_side", "slow_main", "both")
