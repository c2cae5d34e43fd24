"""Flat-buffer AdamW with fused global-norm clipping (reference step: main.py:106-108, optimiser main.py:275).

``FlatParams`` re-homes a module's parameters and gradients into two contiguous f32 buffers
(device-agnostic, pure bookkeeping) so that (a) the optimiser is two kernels -- a sum-of-squares
reduction and one AdamW sweep that reads the clip coefficient on device, no host sync -- and
(b) data-parallel gradient exchange works on contiguous slices (``ddp.FlatDDP``).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import numbers
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch


def build_run_table(sizes: Sequence[int], groups: Sequence[int]) -> List[Tuple[int, int, int]]:
    """Run table of ``uclstm_adamw_step_groups`` for tensors of ``sizes`` elements laid out one after the other, tensor ``i``
    belonging to parameter group ``groups[i]``: ``(begin, end, group)`` element ranges in ascending order that cover
    ``[0, sum(sizes))`` without a gap; neighbouring tensors of the same group are one run.  Pure bookkeeping, no device."""
    if len(sizes) != len(groups):
        raise ValueError("build_run_table: one group index per tensor")
    runs: List[Tuple[int, int, int]] = []
    off = 0
    for n, g in zip(sizes, groups):
        n, g = int(n), int(g)
        if n <= 0 or g < 0:
            raise ValueError("build_run_table: sizes must be positive and group indices non-negative")
        if runs and runs[-1][2] == g:
            runs[-1] = (runs[-1][0], off + n, g)
        else:
            runs.append((off, off + n, g))
        off += n
    return runs


def check_run_table(runs: Sequence[Sequence[int]], n: int, n_groups: int) -> None:
    """Raise ``ValueError`` unless ``runs`` is what the kernel may walk: non-empty runs, the first beginning at 0, each
    beginning where the previous one ends, the last ending at ``n``, every group index in ``[0, n_groups)``.  The library
    cannot check a device table, so this runs on the host before the table is uploaded."""
    if not runs:
        raise ValueError("run table: empty")
    at = 0
    for i, (b, e, g) in enumerate(runs):
        if b != at or e <= b:
            raise ValueError(f"run table: run {i} = [{b}, {e}) does not continue at {at} (runs must be sorted, non-empty and gap-free)")
        if not 0 <= g < n_groups:
            raise ValueError(f"run table: run {i} names group {g}, there are {n_groups}")
        at = e
    if at != n:
        raise ValueError(f"run table: covers [0, {at}), the buffer has {n} elements")


class FlatParams:
    """Parameters and their gradients as views into two flat f32 buffers (registration order)."""

    def __init__(self, params: Iterable[torch.nn.Parameter]):
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FlatParams: no trainable parameters")
        dev, dt = self.params[0].device, self.params[0].dtype
        if dt != torch.float32 or any(p.device != dev or p.dtype != dt for p in self.params):
            raise ValueError("FlatParams: all parameters must be float32 on one device")
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += p.numel()
        self.numel = off
        self.flat_p = torch.empty(off, dtype=dt, device=dev)
        self.flat_g = torch.zeros(off, dtype=dt, device=dev)
        for p, o in zip(self.params, self.offsets):
            self.flat_p[o:o + p.numel()].copy_(p.data.reshape(-1))
            p.data = self.flat_p[o:o + p.numel()].view(p.shape)
        self.attach_grads()

    def attach_grads(self) -> None:
        """(Re)point every ``.grad`` at its slice of the flat buffer (autograd then accumulates in place)."""
        for p, o in zip(self.params, self.offsets):
            g = self.flat_g[o:o + p.numel()].view(p.shape)
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    def zero_grad(self) -> None:
        self.flat_g.zero_()
        self.attach_grads()


def check_ema(decay, warmup, every) -> Tuple[float, float, int]:
    """The arguments of ``FusedAdamW.attach_ema`` as ``(decay, warmup, every)``, or ``ValueError``: ``0 < decay < 1``, ``warmup``
    finite and ``>= 0``, ``every`` an integer ``>= 1`` (below 2^24, where the device-side counts stay exact).  No device."""
    if isinstance(decay, bool) or not isinstance(decay, numbers.Real) or not 0.0 < float(decay) < 1.0:
        raise ValueError(f"attach_ema: decay must be a number with 0 < decay < 1, got {decay!r}")
    if float(torch.tensor(float(decay), dtype=torch.float32)) >= 1.0:
        raise ValueError(f"attach_ema: decay {decay!r} rounds to 1 in float32, the shadow would never move")
    if isinstance(warmup, bool) or not isinstance(warmup, numbers.Real) or not math.isfinite(float(warmup)) or float(warmup) < 0.0:
        raise ValueError(f"attach_ema: warmup must be a finite number >= 0, got {warmup!r}")
    if isinstance(every, bool) or not isinstance(every, numbers.Integral) or not 1 <= every < (1 << 24):
        raise ValueError(f"attach_ema: every must be an integer with 1 <= every < 2^24, got {every!r}")
    return float(decay), float(warmup), int(every)


class WeightEMA:
    """Exponential moving average of an optimiser's weights, kept on the device (``FusedAdamW.attach_ema``).

    ``shadow`` is a flat f32 tensor laid out as ``optimizer.flat.flat_p`` (trainable parameters only); ``state`` is the device
    f32[8] of ``uclstm_ema_update``: ``{decay, warmup, every, steps_seen, updates_done, reserved x 3}``.  Every
    ``optimizer.step()`` ends with one launch of that entry point on the step's stream, so the average follows eager steps,
    captured steps (``engine.GraphedTrainStep``) and the skipped steps of fp16 loss scaling alike, without a host sync.
    Update number ``k`` uses ``min(decay, (1 + k) / (warmup + k))`` (``warmup = 0``: ``decay``), and only every ``every``-th
    applied step updates.  BatchNorm running statistics are not averaged (they are moving averages already)."""

    def __init__(self, optimizer: "FusedAdamW", decay: float, warmup: float, every: int):
        self.optimizer = optimizer
        self.decay, self.warmup, self.every = decay, warmup, every
        flat_p = optimizer.flat.flat_p
        self.shadow = flat_p.detach().clone()
        self.state = torch.tensor([decay, warmup, float(every), 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32).to(flat_p.device)
        self._swapped = False

    def steps_seen(self) -> int:
        """Applied optimiser steps this average has seen (reads the device)."""
        return int(self.state[3].item())

    def updates_done(self) -> int:
        """Updates of the shadow made so far (reads the device)."""
        return int(self.state[4].item())

    def _update(self, sumsq: Optional[torch.Tensor]) -> None:
        from . import _lib as L
        from . import ops
        f = self.optimizer.flat
        if ops.LAUNCH_LOG is not None:
            ops.LAUNCH_LOG.append(("ema", "update", sumsq is not None))
        L.check(L.lib.uclstm_ema_update(C.c_void_p(self.shadow.data_ptr()), C.c_void_p(f.flat_p.data_ptr()), f.numel,
                                        None if sumsq is None else C.c_void_p(sumsq.data_ptr()), C.c_void_p(self.state.data_ptr()),
                                        ops._stream()), "ema_update")

    def _exchange(self) -> None:
        from . import _lib as L
        from . import ops
        f = self.optimizer.flat
        L.check(L.lib.uclstm_swap_f32(C.c_void_p(f.flat_p.data_ptr()), C.c_void_p(self.shadow.data_ptr()), f.numel, ops._stream()),
                "swap_f32")
        ops.weights_changed()          # raw-pointer rewrite of the parameters: the panel caches must be told

    @contextlib.contextmanager
    def swapped(self):
        """Inside the block the model computes with the averaged weights: the CONTENTS of ``flat_p`` and ``shadow`` are
        exchanged in place (``uclstm_swap_f32``, no copy the size of the model) and the panel caches are told
        (``ops.weights_changed()``), on entry and again on exit, also when the block raises.  No address changes, so ``p.data``
        views, gradient views, weight panels and captured graphs stay valid; after the block the weights and the shadow are bit
        for bit what they were.  Not under a graph capture, not nested, and no ``optimizer.step()`` inside."""
        if self._swapped:
            raise RuntimeError("WeightEMA.swapped(): already inside swapped() (it does not nest)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightEMA.swapped() inside a graph capture: exchange the weights outside the captured region")
        self._exchange()
        self._swapped = True
        try:
            yield self
        finally:
            self._swapped = False
            self._exchange()

    @torch.no_grad()
    def model_state_dict(self, model: torch.nn.Module):
        """``model.state_dict()`` with every trainable parameter of the optimiser replaced by its averaged value; everything
        else (frozen parameters, buffers such as the BatchNorm running statistics) as it is.  All entries are clones: the
        result stays valid after the next step, and loads wherever a checkpoint of ``model`` loads."""
        if self._swapped:
            raise RuntimeError("WeightEMA.model_state_dict() inside swapped(): the shadow holds the live weights there")
        f = self.optimizer.flat
        where = {id(p): (o, p.numel()) for p, o in zip(f.params, f.offsets)}
        sd = model.state_dict()
        out = type(sd)((k, v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in sd.items())
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        for name, p in model.named_parameters(remove_duplicate=False):
            if id(p) in where and name in out:
                o, n = where[id(p)]
                out[name] = self.shadow[o:o + n].view(p.shape).clone()
        return out


def build_stat_blocks(sizes: Sequence[int], chunk: int) -> Tuple[np.ndarray, np.ndarray]:
    """The two tables of ``uclstm_param_stats`` for tensors of ``sizes`` elements laid out one after the other: ``blocks`` int64
    ``[n_blocks, 3]`` rows ``{tensor, start, count}`` (``count <= chunk``, no block across two tensors, ordered by tensor and then
    by start) and ``tensor_blocks`` int64 ``[n_tensors, 2]`` rows ``{first_block, n_blocks_of_tensor}``.  Pure bookkeeping, no device."""
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("build_stat_blocks: chunk must be positive")
    if len(sizes) == 0:
        raise ValueError("build_stat_blocks: no tensors")
    blocks: List[Tuple[int, int, int]] = []
    tensors: List[Tuple[int, int]] = []
    off = 0
    for t, n in enumerate(sizes):
        n = int(n)
        if n <= 0:
            raise ValueError(f"build_stat_blocks: tensor {t} has {n} elements (sizes must be positive)")
        first = len(blocks)
        for b in range(0, n, chunk):
            blocks.append((t, off + b, min(chunk, n - b)))
        tensors.append((first, len(blocks) - first))
        off += n
    return np.asarray(blocks, dtype=np.int64).reshape(-1, 3), np.asarray(tensors, dtype=np.int64).reshape(-1, 2)


def check_stat_blocks(blocks, tensor_blocks, n: int, chunk: int) -> None:
    """Raise ``ValueError`` unless the tables are what ``uclstm_param_stats`` may walk: blocks of ``1..chunk`` elements that cover
    ``[0, n)`` in order without a gap, tensor indices that count up from 0 without skipping one, and for every tensor the row
    ``{first_block, n_blocks}`` naming exactly its blocks.  The library cannot check a device table, so this runs on the host
    before the tables are uploaded."""
    blocks, tensor_blocks = np.asarray(blocks), np.asarray(tensor_blocks)
    if blocks.ndim != 2 or blocks.shape[1] != 3 or blocks.shape[0] == 0 or blocks.dtype != np.int64:
        raise ValueError("stat blocks: the block table must be a non-empty int64 [n_blocks, 3]")
    if tensor_blocks.ndim != 2 or tensor_blocks.shape[1] != 2 or tensor_blocks.shape[0] == 0 or tensor_blocks.dtype != np.int64:
        raise ValueError("stat blocks: the tensor table must be a non-empty int64 [n_tensors, 2]")
    at, owner = 0, []
    for i, (t, start, count) in enumerate(blocks.tolist()):
        if not 1 <= count <= chunk:
            raise ValueError(f"stat blocks: block {i} has {count} elements, a block reduces 1..{chunk}")
        if start != at:
            raise ValueError(f"stat blocks: block {i} starts at {start}, not at {at} (blocks must be ordered and gap-free)")
        last = owner[-1] if owner else -1
        if t != last and t != last + 1:
            raise ValueError(f"stat blocks: block {i} names tensor {t} after tensor {last} (ordered by tensor, none skipped)")
        owner.append(t)
        at = start + count
    if at != n:
        raise ValueError(f"stat blocks: the blocks cover [0, {at}), the buffer has {n} elements")
    if owner[-1] + 1 != tensor_blocks.shape[0]:
        raise ValueError(f"stat blocks: the blocks name {owner[-1] + 1} tensors, the tensor table has {tensor_blocks.shape[0]}")
    for t, (first, nb) in enumerate(tensor_blocks.tolist()):
        if nb < 1 or first < 0 or first + nb > len(owner) or any(o != t for o in owner[first:first + nb]) \
                or (first > 0 and owner[first - 1] == t) or (first + nb < len(owner) and owner[first + nb] == t):
            raise ValueError(f"stat blocks: tensor {t}: row {{{first}, {nb}}} does not name exactly its blocks")


def check_monitor(every, history, updates) -> Tuple[int, int, bool]:
    """The arguments of ``FusedAdamW.attach_monitor`` as ``(every, history, updates)``, or ``ValueError``: ``every`` an integer with
    ``1 <= every < 2^24``, ``history`` an integer in ``1..65536``, ``updates`` a bool.  No device."""
    if isinstance(every, bool) or not isinstance(every, numbers.Integral) or not 1 <= every < (1 << 24):
        raise ValueError(f"attach_monitor: every must be an integer with 1 <= every < 2^24, got {every!r}")
    if isinstance(history, bool) or not isinstance(history, numbers.Integral) or not 1 <= history <= 65536:
        raise ValueError(f"attach_monitor: history must be an integer in 1..65536, got {history!r}")
    if not isinstance(updates, bool):
        raise ValueError(f"attach_monitor: updates must be a bool, got {updates!r}")
    return int(every), int(history), updates


class StepMonitor:
    """Per-tensor gradient, weight and update statistics of every ``every``-th ``optimizer.step()``, kept in a ring of ``history``
    records on the device (``FusedAdamW.attach_monitor``).

    Every ``step()`` ends with one call of ``uclstm_param_stats`` on the step's stream: a sweep over ``flat_p``, ``flat_g`` (still
    as the step read it) and ``prev``, the weights at the previous record, which it then overwrites.  Nothing is allocated, copied
    to the host or synchronised, and slot and counts are read from the device, so it records under eager steps, under every
    replay of ``engine.GraphedTrainStep`` and on the skipped steps of fp16 loss scaling alike.  ``read()`` brings the ring to the
    host.  ``state`` is the device int64[8] ``{every, steps_seen, records_done, due, slot, reserved x 3}`` of include/uclstm.h.
    With ``updates=True`` the monitor holds ``prev``, one more f32 copy of the trainable weights (what the EMA's shadow costs);
    with ``updates=False`` it holds none and the update columns read NaN.  A diagnostic: not part of ``optimizer.state_dict()``.
    ``optimizer.load_state_dict`` calls ``reseed()``; after a ``model.load_state_dict`` with a monitor attached, call
    ``reseed()`` yourself, or the next record shows the restore as one huge update."""

    COLS = 8
    PER_TENSOR = ("grad_norm", "grad_max", "grad_nonfinite", "grad_zero_frac", "weight_norm", "weight_max", "weight_nonfinite",
                  "update_norm", "update_ratio")

    def __init__(self, optimizer: "FusedAdamW", every: int, history: int, updates: bool, names: Sequence[str]):
        from . import _lib as L
        self.optimizer = optimizer
        self.every, self.history, self.updates = every, history, updates
        f = optimizer.flat
        dev = f.flat_p.device
        self.names = list(names)
        self.numel = np.asarray([p.numel() for p in f.params], dtype=np.int64)
        self.group = np.asarray(optimizer._tensor_groups, dtype=np.int64)
        self.chunk = int(L.lib.uclstm_param_stats_chunk())
        blocks, tensor_blocks = build_stat_blocks(self.numel.tolist(), self.chunk)
        check_stat_blocks(blocks, tensor_blocks, f.numel, self.chunk)
        self.blocks, self.tensor_blocks = torch.from_numpy(blocks).to(dev), torch.from_numpy(tensor_blocks).to(dev)
        self.partials = torch.zeros((blocks.shape[0], self.COLS), dtype=torch.float64, device=dev)
        self.ring = torch.zeros((history, len(self.names), self.COLS), dtype=torch.float64, device=dev)
        self.meta = torch.zeros((history, 4), dtype=torch.float64, device=dev)
        self.state = torch.tensor([every, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64).to(dev)
        self.prev = f.flat_p.detach().clone() if updates else None

    def steps_seen(self) -> int:
        """Calls of ``optimizer.step()`` this monitor has seen, skipped ones included (reads the device)."""
        return int(self.state[1].item())

    def records_done(self) -> int:
        """Records made so far; the ring holds the last ``history`` of them (reads the device)."""
        return int(self.state[2].item())

    def reseed(self) -> None:
        """``prev = flat_p``: the next record's update column counts from the weights as they are now."""
        if self.prev is not None:
            self.prev.copy_(self.optimizer.flat.flat_p)

    def _record(self, sumsq: Optional[torch.Tensor], scale: Optional[torch.Tensor]) -> None:
        from . import _lib as L
        from . import ops
        f = self.optimizer.flat
        if ops.LAUNCH_LOG is not None:
            ops.LAUNCH_LOG.append(("monitor", "stats", sumsq is not None, scale is not None))
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
        L.check(L.lib.uclstm_param_stats(ptr(f.flat_p), ptr(f.flat_g), ptr(self.prev), f.numel, ptr(self.blocks), int(self.blocks.shape[0]),
                                         ptr(self.tensor_blocks), len(self.names), ptr(self.partials), ptr(self.ring), ptr(self.meta),
                                         self.history, ptr(sumsq), ptr(scale), ptr(self.state), ops._stream()), "param_stats")

    @staticmethod
    def reduce(ring, meta, records_done: int, history: int, updates: bool = True, names: Optional[Sequence[str]] = None,
               numel=None, group=None) -> dict:
        """The report of ``read()`` from host copies of the raw ring f64 ``[history, n, 8]``, meta f64 ``[history, 4]`` and the record
        count: numpy only, no device.  The ``R = min(records_done, history)`` surviving records in chronological order; gradient
        norms and maxima divided by the record's loss scale in f64; ``update_norm`` / ``update_ratio`` NaN without ``updates``."""
        ring = np.asarray(ring, dtype=np.float64).reshape(history, -1, StepMonitor.COLS)
        meta = np.asarray(meta, dtype=np.float64).reshape(history, 4)
        n = ring.shape[1]
        records_done = int(records_done)
        R = max(0, min(records_done, history))
        slots = (records_done - R + np.arange(R)) % history
        rows, m = ring[slots], meta[slots]
        numel = np.ones(n, dtype=np.int64) if numel is None else np.asarray(numel, dtype=np.int64)
        scale = m[:, 1].copy()
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            weight_norm = np.sqrt(rows[:, :, 4])
            update_norm = np.sqrt(rows[:, :, 7]) if updates else np.full((R, n), np.nan)
            out = {
                "step": m[:, 0].astype(np.int64), "skipped": m[:, 3] != 0.0, "scale": scale,
                "global_grad_norm": np.sqrt(m[:, 2]) / scale,
                "names": list(names) if names is not None else [f"param{i}" for i in range(n)],
                "numel": numel, "group": np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64),
                "grad_norm": np.sqrt(rows[:, :, 0]) / scale[:, None], "grad_max": rows[:, :, 1] / scale[:, None],
                "grad_nonfinite": rows[:, :, 2].astype(np.int64), "grad_zero_frac": rows[:, :, 3] / numel[None, :].astype(np.float64),
                "weight_norm": weight_norm, "weight_max": rows[:, :, 5].copy(), "weight_nonfinite": rows[:, :, 6].astype(np.int64),
                "update_norm": update_norm, "update_ratio": update_norm / np.maximum(weight_norm, np.finfo(np.float64).tiny),
            }
        return out

    def read(self) -> dict:
        """The surviving records as numpy arrays, oldest first (one copy of ring, meta and state to the host, then numpy only):
        ``step [R]``, ``skipped [R]`` (bool), ``scale [R]``, ``global_grad_norm [R]`` (NaN where the step computed no global norm),
        ``names``, ``numel [n]``, ``group [n]`` and, ``[R, n]`` each, ``grad_norm``, ``grad_max``, ``grad_nonfinite``, ``grad_zero_frac``,
        ``weight_norm``, ``weight_max``, ``weight_nonfinite``, ``update_norm`` and ``update_ratio = update_norm / max(weight_norm,
        tiny)``.  Gradient norms and maxima are unscaled (divided by the record's loss scale); norms skip non-finite elements,
        which the ``*_nonfinite`` columns count.  ``update_norm`` is the change since the previous record: exactly 0 over
        skipped steps.  ``skipped``: the step's global sum of squares was NaN or infinite, on which the loss-scaling steps skip."""
        state = self.state.cpu().numpy()
        return StepMonitor.reduce(self.ring.cpu().numpy(), self.meta.cpu().numpy(), int(state[2]), self.history, self.updates,
                                  self.names, self.numel, self.group)

    def nonfinite(self, last: int = 1) -> List[Tuple[int, str, int]]:
        """``(step, name, count)`` of every tensor whose gradient held NaN or infinite elements in one of the ``last`` latest
        records: which tensor overflowed an fp16 step."""
        r = self.read()
        out = []
        for k in range(max(0, len(r["step"]) - int(last)), len(r["step"])):
            for i in np.flatnonzero(r["grad_nonfinite"][k] > 0):
                out.append((int(r["step"][k]), r["names"][i], int(r["grad_nonfinite"][k, i])))
        return out

    def report(self, top: int = 8) -> str:
        """A few lines on the latest record: tensors with non-finite gradients, the largest and the smallest ``update_ratio``,
        gradients that are zero in a whole tensor, and per parameter group the pooled ``|dw| / |w|``."""
        r = self.read()
        if len(r["step"]) == 0:
            return "StepMonitor: no record yet"
        k, names = len(r["step"]) - 1, r["names"]
        lines = [f"StepMonitor: step {int(r['step'][k])}{' (skipped)' if r['skipped'][k] else ''}, loss scale {r['scale'][k]:g}, "
                 f"global grad norm {r['global_grad_norm'][k]:.4g}, {len(names)} tensors"]
        bad = np.flatnonzero(r["grad_nonfinite"][k] > 0)
        lines.append(f"  non-finite gradients: {len(bad)} tensors" + "".join(
            f"\n    {names[i]}: {int(r['grad_nonfinite'][k, i])} of {int(r['numel'][i])}" for i in bad[:top]))
        if self.updates:
            ratio = r["update_ratio"][k]
            order = np.argsort(ratio, kind="stable")
            for title, pick in (("largest", order[::-1][:top]), ("smallest", order[:top])):
                lines.append(f"  {title} |dw| / |w| since the previous record:" + "".join(
                    f"\n    {names[i]}: {ratio[i]:.3e}" for i in pick))
        dead = np.flatnonzero(r["grad_zero_frac"][k] == 1.0)
        lines.append(f"  all-zero gradients: {len(dead)} tensors" + "".join(f"\n    {names[i]}" for i in dead[:top]))
        for gi in sorted(set(r["group"].tolist())):
            sel = r["group"] == gi
            w = math.sqrt(float(np.sum(r["weight_norm"][k, sel] ** 2)))
            line = f"  group {gi}: {int(sel.sum())} tensors, {int(r['numel'][sel].sum())} elements, |w| {w:.4g}"
            if self.updates:
                line += f", pooled |dw| / |w| {math.sqrt(float(np.sum(r['update_norm'][k, sel] ** 2))) / max(w, np.finfo(np.float64).tiny):.3e}"
            lines.append(line)
        return "\n".join(lines)


class FusedAdamW(torch.optim.Optimizer):
    """AdamW(lr, betas, eps, weight_decay) + optional ``clip_grad_norm_(max_grad_norm)`` in two HIP kernels.

    Semantics equal ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` followed by
    ``torch.optim.AdamW.step()`` (main.py:106-108).  ``zero_grad`` keeps gradients as views of the
    flat buffer (``set_to_none`` is accepted and ignored).

    ``params`` may be parameter groups with their own ``lr``, ``betas``, ``eps`` and ``weight_decay`` (``max_grad_norm`` stays
    global: one norm over all trainable parameters).  All groups live in ONE flat buffer, laid out as ``order`` says (any
    iterable of parameters, normally ``model.parameters()``: the layout of the single-group optimiser of that model, which
    is what ``ddp.FlatDDP``'s bucket order is built on), else group after group.  Parameters with ``requires_grad=False`` are
    left out.  More than one group, or ``capturable`` together with ``loss_scale``, runs ``uclstm_adamw_step_groups`` (one
    sweep, a device table of runs, a device table of hyper-parameters); a single group keeps the entry points it always used.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm: Optional[float] = None,
                 loss_scale: Optional[float] = None, scale_growth: float = 2.0, scale_backoff: float = 0.5, scale_interval: int = 2000,
                 capturable: bool = False, order: Optional[Iterable[torch.nn.Parameter]] = None):
        params = list(params)
        self._laid_out = False
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        if order is None:
            seq = [p for g in self.param_groups for p in g["params"]]
        else:
            seq = list(order)
            if len({id(p) for p in seq}) != len(seq):
                raise ValueError("FusedAdamW: a parameter appears twice in `order`")
            if any(p.requires_grad and id(p) not in group_of for p in seq):
                raise ValueError("FusedAdamW: a trainable parameter of `order` is in no parameter group")
            missing = set(group_of) - {id(p) for p in seq}
            if missing:
                raise ValueError(f"FusedAdamW: {len(missing)} parameters of the groups are not in `order`")
        self.flat = FlatParams(seq)
        self._laid_out = True                       # the flat buffers exist: no add_param_group from here on
        if not self.flat.flat_p.is_cuda:
            raise RuntimeError("FusedAdamW needs HIP device parameters (no CPU path)")
        self._tensor_groups = [group_of[id(p)] for p in self.flat.params]
        self.m = torch.zeros_like(self.flat.flat_p)
        self.v = torch.zeros_like(self.flat.flat_p)
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=self.flat.flat_p.device)
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        self.ema: Optional[WeightEMA] = None        # attach_ema()
        self.monitor: Optional[StepMonitor] = None  # attach_monitor()
        # fp16 compute (ops.compute_dtype(torch.float16)): dynamic loss scaling, all on the device.  ``scale_state`` =
        # [scale, growth tracker, successful steps]; the training step multiplies the loss by scale_state[0] before backward.
        self.scale_state = None
        self._scale_cfg = (float(scale_growth), float(scale_backoff), int(scale_interval))
        if loss_scale is not None:
            self.scale_state = torch.tensor([float(loss_scale), 0.0, 0.0], dtype=torch.float32, device=self.flat.flat_p.device)
        # capturable: hyper-parameters and the step count live on the device (uclstm_adamw_step_dev), so that step() makes the
        # same launches with the same arguments every time and can be captured in a HIP graph (engine.GraphedTrainStep); a
        # changed lr / max_grad_norm reaches the device through one small copy in sync_hyper(), outside the graph.
        self.capturable = bool(capturable)
        self.hyper = None
        # Parameter groups, and a captured step with loss scaling: uclstm_adamw_step_groups.  ``runs`` = i64 [n_runs, 3]
        # (begin, end, group) over the flat buffer, ``group_hyper`` = f32 [1 + groups, 8]: row 0 {max_norm, steps done}, row
        # 1 + k {lr, beta1, beta2, eps, weight_decay} of group k (include/uclstm.h).  Also in eager mode: one implementation.
        self.uses_groups = len(self.param_groups) > 1 or (self.capturable and loss_scale is not None)
        self.runs = self.group_hyper = None
        if self.uses_groups:
            dev = self.flat.flat_p.device
            table = build_run_table([p.numel() for p in self.flat.params], self._tensor_groups)
            check_run_table(table, self.flat.numel, len(self.param_groups))
            self.runs = torch.tensor(table, dtype=torch.int64).to(dev)
            self.group_hyper = torch.zeros((1 + len(self.param_groups), 8), dtype=torch.float32, device=dev)
            self._last_scale = torch.ones((), dtype=torch.float32, device=dev)
            self._hyper_host = (None, None)
            self.sync_hyper()
        elif self.capturable:
            self.hyper = torch.zeros(8, dtype=torch.float32, device=self.flat.flat_p.device)
            self._hyper_host = None
            self.sync_hyper()

    def add_param_group(self, param_group) -> None:
        if getattr(self, "_laid_out", False):
            raise RuntimeError("FusedAdamW.add_param_group: the flat buffers are laid out once, in __init__; build a new optimiser")
        super().add_param_group(param_group)

    def attach_ema(self, decay: float = 0.999, warmup: float = 10.0, every: int = 1) -> WeightEMA:
        """Keep an exponential moving average of the weights on the device (``WeightEMA``): from now on every ``step()`` ends
        with one ``uclstm_ema_update`` sweep on its stream.  Called once, after construction; the shadow starts as a copy of the
        current weights.  Update number ``k`` uses the decay ``min(decay, (1 + k) / (warmup + k))`` (``warmup=0``: always
        ``decay``), and only every ``every``-th applied step updates.  A step that fp16 loss scaling skips is not seen."""
        decay, warmup, every = check_ema(decay, warmup, every)
        if getattr(self, "ema", None) is not None:
            raise RuntimeError("FusedAdamW.attach_ema: an EMA is attached already")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW.attach_ema() inside a graph capture")
        self.ema = WeightEMA(self, decay, warmup, every)
        return self.ema

    def attach_monitor(self, every: int = 1, history: int = 128, updates: bool = True, names=None) -> StepMonitor:
        """Record per-tensor statistics of the gradients, the weights and the update on the device (``StepMonitor``): from now on
        every ``step()`` ends with one ``uclstm_param_stats`` call on its stream, which records every ``every``-th step into a ring
        of ``history`` records.  Called once, after construction.  ``names``: ``model.named_parameters()`` or any iterable of
        ``(name, parameter)``, matched by identity against the optimiser's trainable tensors; a tensor without a name is
        ``param{i}``.  ``updates=True`` holds one more f32 copy of the trainable weights (``prev``, the memory of an EMA shadow) for
        the ``|dw| / |w|`` columns; ``updates=False`` holds none and those columns read NaN.  Tables, scratch, ring and state are
        allocated here, nothing in ``step()``."""
        every, history, updates = check_monitor(every, history, updates)
        if getattr(self, "monitor", None) is not None:
            raise RuntimeError("FusedAdamW.attach_monitor: a monitor is attached already")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW.attach_monitor() inside a graph capture")
        given = {id(p): str(n) for n, p in names} if names is not None else {}
        self.monitor = StepMonitor(self, every, history, updates, [given.get(id(p), f"param{i}") for i, p in enumerate(self.flat.params)])
        return self.monitor

    def _group_values(self):
        return tuple((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
                     for g in self.param_groups)

    def steps_done(self) -> int:
        """Optimiser steps applied so far (with loss scaling: the successful ones, ``scale_state[2]``; ``step_count`` also counts
        the skipped ones).  Reads the device where the count lives."""
        if self.scale_state is not None:
            return int(self.scale_state[2].item())
        if self.uses_groups:
            return int(self.group_hyper[0, 1].item())
        if self.capturable:
            return int(self.hyper[6].item())
        return int(self.step_count)

    def _hyper_values(self):
        g = self.param_groups[0]
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                float(self.max_grad_norm or 0.0))

    def sync_hyper(self) -> None:
        """Push lr / betas / eps / weight_decay / max_grad_norm to the device if they changed (capturable mode; never inside a
        capture).  The device-side step count is left alone.  With parameter groups: every group's values."""
        if self.uses_groups:
            vals, mx = self._group_values(), float(self.max_grad_norm or 0.0)
            if (vals, mx) != self._hyper_host:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("FusedAdamW.sync_hyper() inside a graph capture: hyper-parameters must be synchronised before")
                if vals != self._hyper_host[0]:
                    self.group_hyper[1:, :5].copy_(torch.tensor(vals, dtype=torch.float32))
                if mx != self._hyper_host[1]:
                    self.group_hyper[0, :1].copy_(torch.tensor([mx], dtype=torch.float32))
                self._hyper_host = (vals, mx)
            return
        if not self.capturable:
            return
        vals = self._hyper_values()
        if vals != self._hyper_host:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW.sync_hyper() inside a graph capture: hyper-parameters must be synchronised before")
            self.hyper[:6].copy_(torch.tensor(vals, dtype=torch.float32))
            self._hyper_host = vals

    def zero_grad(self, set_to_none: bool = False) -> None:   # noqa: ARG002 - signature parity with torch
        self.flat.zero_grad()

    # The moments and the bias-correction step live in flat buffers outside ``Optimizer.state``: carry them explicitly,
    # otherwise a save / load / resume would silently restart Adam.
    def state_dict(self):
        sd = super().state_dict()
        if self.capturable or self.uses_groups or self.scale_state is not None:
            self.step_count = self.steps_done()                  # the device-side count is the truth wherever there is one
        sd["fused"] = {"exp_avg": self.m.detach().clone(), "exp_avg_sq": self.v.detach().clone(), "step": int(self.step_count),
                       "numel": int(self.flat.numel),
                       "scale_state": None if self.scale_state is None else self.scale_state.detach().clone(),
                       # the layout of the flat buffers: a state saved with another grouping or order must not be loaded
                       "sizes": [int(p.numel()) for p in self.flat.params], "tensor_groups": list(self._tensor_groups)}
        if self.ema is not None:
            if self.ema._swapped:
                raise RuntimeError("FusedAdamW.state_dict() inside WeightEMA.swapped(): the shadow holds the live weights there")
            sd["fused"]["ema"] = {"shadow": self.ema.shadow.detach().clone(), "state": self.ema.state.detach().clone()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        fused = state_dict.get("fused")
        if fused is None:
            raise ValueError("FusedAdamW.load_state_dict: no 'fused' entry (not a FusedAdamW state_dict)")
        if int(fused["numel"]) != self.flat.numel:
            raise ValueError(f"FusedAdamW.load_state_dict: {fused['numel']} parameters saved, {self.flat.numel} here")
        if "tensor_groups" in fused:
            if (list(fused["tensor_groups"]) != list(self._tensor_groups)
                    or list(fused["sizes"]) != [int(p.numel()) for p in self.flat.params]):
                raise ValueError("FusedAdamW.load_state_dict: the state was saved with another parameter grouping / layout")
        elif len(self.param_groups) != 1:
            raise ValueError("FusedAdamW.load_state_dict: a single-group state cannot be loaded into parameter groups")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "fused"})
        self.m.copy_(fused["exp_avg"])
        self.v.copy_(fused["exp_avg_sq"])
        self.step_count = int(fused["step"])
        if self.uses_groups:
            self.group_hyper[0, 1] = float(self.step_count)
        elif self.capturable:
            self.hyper[6] = float(self.step_count)
        if fused.get("scale_state") is not None and self.scale_state is not None:
            self.scale_state.copy_(fused["scale_state"])
        # The weight EMA.  A state with "ema" restores the shadow and all of its device state (decay, warm-up, period and both
        # counts); a state WITHOUT it re-seeds the shadow from the weights as they are at this moment (load the model first)
        # and zeroes the counts, so the warm-up starts over.  An "ema" entry is ignored by an optimiser that has none attached.
        if self.ema is not None:
            ema = self.ema
            if ema._swapped:
                raise RuntimeError("FusedAdamW.load_state_dict() inside WeightEMA.swapped()")
            saved = fused.get("ema")
            if saved is not None:
                if saved["shadow"].numel() != self.flat.numel or saved["state"].numel() != ema.state.numel():
                    raise ValueError("FusedAdamW.load_state_dict: the saved EMA does not fit this optimiser's flat buffer")
                ema.shadow.copy_(saved["shadow"])
                ema.state.copy_(saved["state"])
                decay, warmup, every = (float(v) for v in ema.state[:3].tolist())
                ema.decay, ema.warmup, ema.every = decay, warmup, int(every)
            else:
                ema.shadow.copy_(self.flat.flat_p)
                ema.state[3:5] = 0.0
        if getattr(self, "monitor", None) is not None:      # a restore is not an update: the next record counts from here
            self.monitor.reseed()

    @torch.no_grad()
    def grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the last step's (unscaled) gradients (device scalar, f64)."""
        n = self.sumsq.sqrt()
        return n if self.scale_state is None else n / self._last_scale.double()

    def scale_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """The tensor to call ``backward()`` on: ``loss`` itself, or ``loss * scale`` with fp16 loss scaling."""
        return loss if self.scale_state is None else loss * self.scale_state[0]

    def _global_sumsq(self) -> None:
        """self.sumsq = sum of squares of the flat gradient buffer (the global norm the clip coefficient comes from).  In
        deterministic mode the block totals go through a partial buffer and are added in a fixed order; nothing is zeroed."""
        from . import _lib as L
        from . import ops
        f = self.flat
        if ops.is_deterministic():
            partials = torch.empty(int(L.lib.uclstm_sumsq_ordered_rows(f.numel)), dtype=torch.float64, device=f.flat_g.device)
            ops._log_reduce("sumsq_ordered")
            L.check(L.lib.uclstm_sumsq_ordered(C.c_void_p(f.flat_g.data_ptr()), f.numel, C.c_void_p(partials.data_ptr()),
                                               C.c_void_p(self.sumsq.data_ptr()), 0, ops._stream()), "sumsq_ordered")
            return
        self.sumsq.zero_()
        ops._log_reduce("sumsq")
        L.check(L.lib.uclstm_sumsq(C.c_void_p(f.flat_g.data_ptr()), f.numel, C.c_void_p(self.sumsq.data_ptr()), ops._stream()), "sumsq")

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib as L
        from .ops import _stream
        assert closure is None
        ema = self.ema
        if ema is not None and ema._swapped:
            raise RuntimeError("FusedAdamW.step() inside WeightEMA.swapped(): the parameters hold the averaged weights there")
        monitor = self.monitor
        g = self.param_groups[0]
        f = self.flat
        f.attach_grads()
        self.step_count += 1
        if self.uses_groups:
            if not torch.cuda.is_current_stream_capturing():
                self.sync_hyper()
            self._global_sumsq()
            state = None
            if self.scale_state is not None:
                self._last_scale.copy_(self.scale_state[0])      # a buffer of its own: the scale update below overwrites the state
                state = C.c_void_p(self.scale_state.data_ptr())
            L.check(L.lib.uclstm_adamw_step_groups(C.c_void_p(f.flat_p.data_ptr()), C.c_void_p(self.m.data_ptr()), C.c_void_p(self.v.data_ptr()),
                                                   C.c_void_p(f.flat_g.data_ptr()), f.numel, C.c_void_p(self.sumsq.data_ptr()),
                                                   C.c_void_p(self.runs.data_ptr()), int(self.runs.shape[0]),
                                                   C.c_void_p(self.group_hyper.data_ptr()), len(self.param_groups), state, _stream()),
                    "adamw_step_groups")
            if state is not None:
                gr, bo, it = self._scale_cfg
                L.check(L.lib.uclstm_loss_scale_update(state, C.c_void_p(self.sumsq.data_ptr()), gr, bo, it, _stream()), "loss_scale_update")
            if ema is not None:
                ema._update(self.sumsq if state is not None else None)          # only a scaled step can have been skipped
            if monitor is not None:
                monitor._record(self.sumsq, self._last_scale if state is not None else None)
            from . import ops
            ops.weights_changed()
            return None
        if self.scale_state is not None:
            self._last_scale = self.scale_state[0].clone()
            self._global_sumsq()
            L.check(L.lib.uclstm_adamw_step_scaled(C.c_void_p(f.flat_p.data_ptr()), C.c_void_p(self.m.data_ptr()), C.c_void_p(self.v.data_ptr()),
                                                   C.c_void_p(f.flat_g.data_ptr()), f.numel, C.c_void_p(self.sumsq.data_ptr()),
                                                   float(self.max_grad_norm or 0.0), float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                                                   float(g["eps"]), float(g["weight_decay"]), C.c_void_p(self.scale_state.data_ptr()), _stream()),
                    "adamw_step_scaled")
            gr, bo, it = self._scale_cfg
            L.check(L.lib.uclstm_loss_scale_update(C.c_void_p(self.scale_state.data_ptr()), C.c_void_p(self.sumsq.data_ptr()), gr, bo, it,
                                                   _stream()), "loss_scale_update")
            if ema is not None:
                ema._update(self.sumsq)
            if monitor is not None:
                monitor._record(self.sumsq, self._last_scale)
            from . import ops
            ops.weights_changed()
            return None
        if self.capturable:
            if not torch.cuda.is_current_stream_capturing():
                self.sync_hyper()
            self._global_sumsq()
            L.check(L.lib.uclstm_adamw_step_dev(C.c_void_p(f.flat_p.data_ptr()), C.c_void_p(self.m.data_ptr()), C.c_void_p(self.v.data_ptr()),
                                                C.c_void_p(f.flat_g.data_ptr()), f.numel, C.c_void_p(self.sumsq.data_ptr()),
                                                C.c_void_p(self.hyper.data_ptr()), _stream()), "adamw_step_dev")
            if ema is not None:
                ema._update(None)
            if monitor is not None:
                monitor._record(self.sumsq, None)
            from . import ops
            ops.weights_changed()
            return None
        sq = None
        if self.max_grad_norm is not None:
            self._global_sumsq()
            sq = C.c_void_p(self.sumsq.data_ptr())
        L.check(L.lib.uclstm_adamw_step(C.c_void_p(f.flat_p.data_ptr()), C.c_void_p(self.m.data_ptr()), C.c_void_p(self.v.data_ptr()),
                                        C.c_void_p(f.flat_g.data_ptr()), f.numel, sq,
                                        float(self.max_grad_norm or 0.0), float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                                        float(g["eps"]), float(g["weight_decay"]), self.step_count, _stream()), "adamw_step")
        if ema is not None:
            ema._update(None)
        if monitor is not None:
            monitor._record(self.sumsq if sq is not None else None, None)
        from . import ops
        ops.weights_changed()          # raw-pointer update: tensor versions do not move, panel caches must be told
        return None
