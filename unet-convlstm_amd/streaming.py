"""Stateful frame-by-frame inference (SURVEY.md section 8f-4 / BASELINE.json config 5).

The reference's inference script re-runs the model on growing prefixes (test.py:305-310: O(T^2) frames, no carried
state).  ``StreamingPredictor`` keeps every recurrent state (temporal AND skip LSTMs) on the device and advances one
frame per call; with ``use_graph=True`` the whole step -- encoder, three ConvLSTM cell steps, decoder, state update --
is captured into a HIP graph (one per state parity: the hidden states alternate between two buffer sets, the cell
states are updated in place, so carrying the state costs no copies) and replayed: a step is one graph launch instead of
~70 kernel launches.

``PretrainedStreamingPredictor`` is the same for the shipped model, ``resnet.PretrainedTemporalUNet``: five recurrences of
``lstm_layers`` layers each, stepped layer by layer through ``ops.convlstm_tick``.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import UclstmError
from .modules import TemporalUNetDualView
from .resnet import ENCODER_CHANNELS, PretrainedTemporalUNet


class _StreamingBase:
    """What the two predictors share: two state sets (frame n reads set [n & 1] and writes the other; the cell states are one
    tensor in both), one captured step per parity, a PanelCache of its own, and dropping graphs and panels when the weights
    change.  A subclass says which model it drives (``_check_model``), what a frame must look like (``_check_frame``) and
    what the state is (``_state_spec``); the model's ``step_nhwc(x_t, state, out_state)`` is the step."""

    def __init__(self, model, use_graph: bool = True, warmup: int = 2):
        self._check_model(model)
        self.model = model.eval()
        self.use_graph = use_graph
        self.warmup = warmup
        self.reset()

    def _check_model(self, model) -> None:
        raise NotImplementedError

    def _check_frame(self, x_t) -> None:
        pass

    def _state_spec(self, x_t: torch.Tensor) -> dict:
        """``{name: (padded channels, h, w, layers)}`` of the recurrent states for frames like ``x_t``."""
        raise NotImplementedError

    def reset(self) -> None:
        """Forget the recurrent state (next frame starts a new sequence), any captured graph and the packed panels."""
        self._states: Optional[list] = None          # two state sets: frame n reads [n & 1] and writes [1 - (n & 1)]
        self._parity = 0
        self._shape = None
        self._drop_graph_and_panels()

    def new_sequence(self) -> None:
        """Zero the recurrent state IN PLACE (the captured graphs keep updating these very buffers): the next frame starts a
        new sequence of the same shape, the graphs and the packed panels stay."""
        if self._states is not None:
            for st in self._states:
                for layers in st.values():
                    for h, c in layers:
                        h.zero_()
                        c.zero_()

    @property
    def state(self) -> Optional[dict]:
        """The current recurrent state: ``{name: [(h NHWC, c f32 NHWC) per layer]}`` (live buffers)."""
        return None if self._states is None else self._states[self._parity]

    def _drop_graph_and_panels(self) -> None:
        # order matters: the captured graph has the panels' addresses baked in, so it goes first; the panels are owned by
        # this predictor's cache (never by a module-global one) and die with it
        self._graphs = [None, None]                   # one captured step per state parity
        self._static_x = None
        self._static_y = [None, None]
        self._eager_steps = 0
        self._panels = ops.PanelCache()
        self._wsig = self._weights_signature()

    def _weights_signature(self):
        return (ops.WEIGHTS_EPOCH, sum(p._version for p in self.model.parameters()) + sum(b._version for b in self.model.buffers()))

    # ---- state: fixed buffers so that captured graphs can update them in place, and no copies: the cell state c is updated
    #      in place (the cell update is element-wise), the hidden state h alternates between two buffers (the gate convolution
    #      reads h_{t-1}'s neighbourhoods while h_t is written).  Frames of even parity read set 0 and write set 1.
    def _zero_states(self, x_t: torch.Tensor) -> list:
        dev, B = x_t.device, x_t.shape[0]
        sets = [{}, {}]
        for name, (chp, h, w, n_layers) in self._state_spec(x_t).items():
            cs = [torch.zeros((B, h, w, chp), dtype=torch.float32, device=dev) for _ in range(n_layers)]
            for st in sets:
                st[name] = [(torch.zeros((B, h, w, chp), dtype=ops.get_compute_dtype(), device=dev), cs[i]) for i in range(n_layers)]
        return sets

    def _eager(self, x_t: torch.Tensor, parity: int) -> torch.Tensor:
        y, _ = self.model.step_nhwc(x_t, self._states[parity], self._states[1 - parity])
        return y

    @torch.no_grad()
    def step(self, x_t: torch.Tensor) -> torch.Tensor:
        """One frame ``[B, C, H, W]`` (f32, device) -> prediction ``[B, out, H, W]`` (a fresh tensor)."""
        self._check_frame(x_t)
        x_t = x_t.contiguous().float()
        if self._shape != tuple(x_t.shape):
            if self._shape is not None:
                raise ValueError(f"{type(self).__name__}: frame shape changed; call reset() first")
            self._shape = tuple(x_t.shape)
            self._states = self._zero_states(x_t)
            self._parity = 0
        sig = self._weights_signature()
        if self._panels.stale() or sig != self._wsig:
            # the model was trained on (fused optimiser step, or any in-place update that bumped a tensor version) since the
            # panels were packed: keep the recurrent state, drop everything that holds old weights
            self._drop_graph_and_panels()
            self._wsig = sig
        p = self._parity
        self._parity = 1 - p
        with self._panels:                            # weights are frozen between optimiser steps: pack each panel once
            if not self.use_graph:
                return self._eager(x_t, p)
            if self._graphs[p] is None:
                if self._eager_steps < self.warmup:   # eager warm-up: first-launch attribute calls, panel cache fill
                    self._eager_steps += 1
                    return self._eager(x_t, p)
                if self._static_x is None:
                    self._static_x = x_t.clone()
                else:
                    self._static_x.copy_(x_t)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._static_y[p] = self._eager(self._static_x, p)
                self._graphs[p] = g
                # the capture only RECORDED the step for x_t: replay it now so that this frame is actually consumed
            self._static_x.copy_(x_t)
            self._graphs[p].replay()
            return self._static_y[p].clone()

    @torch.no_grad()
    def rollout(self, x_seq: torch.Tensor) -> torch.Tensor:
        """``[B, T, C, H, W]`` -> ``[B, T, out, H, W]`` frame by frame from the current state."""
        return torch.stack([self.step(x_seq[:, t]) for t in range(x_seq.shape[1])], dim=1)


class StreamingPredictor(_StreamingBase):
    """Frame-by-frame inference of a ``TemporalUNetDualView``; ``state`` has the keys ``'temporal' | 'skip3' | 'skip2'``."""

    def __init__(self, model: TemporalUNetDualView, use_graph: bool = True, warmup: int = 2):
        super().__init__(model, use_graph, warmup)

    def _check_model(self, model) -> None:
        if not isinstance(model, TemporalUNetDualView):
            # the step it captures is TemporalUNetDualView.step_nhwc with its three recurrent states; the shipped model has
            # a predictor of its own (PretrainedStreamingPredictor)
            raise TypeError(f"StreamingPredictor drives a TemporalUNetDualView, got {type(model).__name__} "
                            "(PretrainedTemporalUNet has no frame-by-frame step)")

    def _state_spec(self, x_t: torch.Tensor) -> dict:
        m = self.model
        _, _, H, W = x_t.shape
        c = m.base_ch
        spec = {"temporal": (ops.cpad(c * 16), H // 16, W // 16, len(m.temporal.layers))}
        if m.use_skip_lstm:
            spec["skip3"] = (ops.cpad(c * 8), H // 8, W // 8, 1)
            spec["skip2"] = (ops.cpad(c * 4), H // 4, W // 4, 1)
        return spec


class PretrainedStreamingPredictor(_StreamingBase):
    """Frame-by-frame inference of a ``PretrainedTemporalUNet`` (the reference's shipped model): what test.py's prefix loop
    computes, one frame of work per frame.  ``state`` has the keys ``'lstm'`` and ``'skip1'`` .. ``'skip4'``, ``lstm_layers``
    entries each.  Frames are f32 ``[B, 2, H, W]`` on the device with H and W multiples of 32."""

    def __init__(self, model: PretrainedTemporalUNet, use_graph: bool = True, warmup: int = 2):
        super().__init__(model, use_graph, warmup)

    def _check_model(self, model) -> None:
        if not isinstance(model, PretrainedTemporalUNet):
            raise TypeError(f"PretrainedStreamingPredictor drives a PretrainedTemporalUNet, got {type(model).__name__}"
                            + (" (StreamingPredictor drives that model)" if isinstance(model, TemporalUNetDualView) else ""))

    def _check_frame(self, x_t) -> None:
        if not isinstance(x_t, torch.Tensor) or not x_t.is_cuda:
            raise UclstmError("PretrainedStreamingPredictor: a HIP device tensor is required (this package has no CPU path)")
        if x_t.dim() != 4 or x_t.shape[1] != ENCODER_CHANNELS[0] or x_t.shape[2] % 32 or x_t.shape[3] % 32:
            raise UclstmError(f"PretrainedStreamingPredictor: frames are [B, {ENCODER_CHANNELS[0]}, H, W] with H and W multiples "
                              f"of 32, got {tuple(x_t.shape)}")
        if self.model.training:
            # a replayed graph would not notice; step_nhwc itself checks every BatchNorm whenever it runs eagerly
            raise UclstmError("PretrainedStreamingPredictor: the model is in training mode; call model.eval() first")

    def _state_spec(self, x_t: torch.Tensor) -> dict:
        B, _, H, W = x_t.shape
        return {key: (shape[3], shape[1], shape[2], n_layers) for key, (n_layers, shape) in self.model.state_spec(B, H, W).items()}
