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
        from . import ops
        ops.weights_changed()          # raw-pointer update: tensor versions do not move, panel caches must be told
        return None
