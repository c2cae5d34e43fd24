"""compute_loss of the reference's main.py:28-72 as one fused HIP reduction (+ one backward kernel), and ``LossSpec``: the same
kernels with the point term (L1 / L2 / Huber), the weight and the gradient term's coefficient as parameters, and
``WeightedLossSpec``: a LossSpec with a weight per frame and per target channel."""
from __future__ import annotations

import dataclasses
import math

import torch

from . import ops

_POINTS = ("l1", "l2", "huber")


def _real(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"LossSpec.{name} must be a real number, got {v!r}")
    return float(v)


@dataclasses.dataclass(frozen=True)
class LossSpec:
    """``loss = point + grad_weight * gradient term`` with ``d = y_pred - y``:

    * ``point``: ``rho(d)`` is ``|d|`` (``"l1"``), ``d^2`` (``"l2"``) or Huber (``"huber"``: ``0.5 d^2`` where ``|d| <= delta``, else
      ``delta (|d| - 0.5 delta)``); ``delta`` is read by Huber alone;
    * ``w = 1 + weight_gain * |y|^weight_power``; masked the point term is ``sum(rho w m) / (sum(w m) + eps)``, unmasked
      ``mean(rho w)`` (main.py:40-45);
    * the gradient term is main.py:47-68 unchanged (L1 on the forward differences, ``eps`` in its masked denominator);
      ``grad_weight == 0`` removes it altogether: no neighbour is read, and a one-row or one-column plane has a finite loss.

    The defaults are the reference's loss (``LossSpec.reference()``), which runs on the kernels it always ran on."""
    point: str = "l1"
    delta: float = 1.0
    weight_gain: float = 4.0
    weight_power: int = 3
    grad_weight: float = 0.005
    eps: float = 1e-8

    def __post_init__(self):
        if self.point not in _POINTS:
            raise ValueError(f"LossSpec.point must be one of {_POINTS}, got {self.point!r}")
        delta, gain, gw, eps = (_real(getattr(self, n), n) for n in ("delta", "weight_gain", "grad_weight", "eps"))
        if self.point == "huber" and not (delta > 0 and math.isfinite(delta)):
            raise ValueError(f"LossSpec.delta must be positive and finite, got {self.delta!r}")
        if not (gain >= 0 and math.isfinite(gain)):
            raise ValueError(f"LossSpec.weight_gain must be >= 0 and finite, got {self.weight_gain!r}")
        if isinstance(self.weight_power, bool) or not isinstance(self.weight_power, int) or not 1 <= self.weight_power <= 4:
            raise ValueError(f"LossSpec.weight_power must be an integer 1..4, got {self.weight_power!r}")
        if not (gw >= 0 and math.isfinite(gw)):
            raise ValueError(f"LossSpec.grad_weight must be >= 0 and finite, got {self.grad_weight!r}")
        if not eps > 0:
            raise ValueError(f"LossSpec.eps must be positive, got {self.eps!r}")

    @classmethod
    def reference(cls) -> "LossSpec":
        """main.py:28-72: weighted L1 (1 + 4|y|^3) + 0.005 x gradient L1, 1e-8 in the denominators."""
        return cls()

    @classmethod
    def masked_mse(cls, eps: float = 1e-6) -> "LossSpec":
        """train/overfit_check.py:106-107: ``((y_pred - y)^2 * mask).sum() / (mask.sum() + eps)``."""
        return cls(point="l2", weight_gain=0.0, grad_weight=0.0, eps=eps)

    @property
    def is_reference(self) -> bool:
        """Every field equals the reference's: such a spec takes the reference's own entry points."""
        return self == _REFERENCE


_REFERENCE = LossSpec()


def _weights(v, name):
    """A weight tuple of WeightedLossSpec: None, or real numbers >= 0 and finite with at least one positive one."""
    if v is None:
        return None
    if not isinstance(v, (tuple, list)):
        raise ValueError(f"WeightedLossSpec.{name} must be a tuple of real numbers or None, got {v!r}")
    out = []
    for e in v:
        if isinstance(e, bool) or not isinstance(e, (int, float)) or not (e >= 0 and math.isfinite(e)):
            raise ValueError(f"WeightedLossSpec.{name} entries must be real numbers >= 0 and finite, got {e!r}")
        out.append(float(e))
    if not any(e > 0 for e in out):
        raise ValueError(f"WeightedLossSpec.{name} needs at least one positive entry, got {v!r}")
    return tuple(out)


@dataclasses.dataclass(frozen=True)
class WeightedLossSpec(LossSpec):
    """A ``LossSpec`` with a weight per frame and per target channel.  For ``y [B,T,Cy,H,W]`` the plane of frame ``t`` and channel
    ``c`` counts ``q = f32(frame_weights[t] * channel_weights[c])`` times in each of the four sums of the loss (a missing tuple is
    all ones): masked ``sum(rho w m q) / (sum(w m q) + eps)``, unmasked the same with ``m = 1`` and the exact denominator, and the
    gradient term likewise.  Scaling all weights by a constant leaves the loss unchanged (up to ``eps``); with both tuples None the
    spec is its ``base`` in every respect."""
    frame_weights: "tuple | None" = None
    channel_weights: "tuple | None" = None

    def __post_init__(self):
        super().__post_init__()
        object.__setattr__(self, "frame_weights", _weights(self.frame_weights, "frame_weights"))
        object.__setattr__(self, "channel_weights", _weights(self.channel_weights, "channel_weights"))

    @classmethod
    def burn_in(cls, T: int, skip: int, **spec_fields) -> "WeightedLossSpec":
        """The first ``skip`` of ``T`` frames do not count (a ConvLSTM has no history at t = 0), the others count alike."""
        if isinstance(T, bool) or isinstance(skip, bool) or not isinstance(T, int) or not isinstance(skip, int) or not 0 <= skip < T:
            raise ValueError(f"burn_in needs integers 0 <= skip < T, got T={T!r}, skip={skip!r}")
        return cls(frame_weights=(0.0,) * skip + (1.0,) * (T - skip), **spec_fields)

    @classmethod
    def last_frames(cls, T: int, keep: int, **spec_fields) -> "WeightedLossSpec":
        """Only the last ``keep`` of ``T`` frames count."""
        if isinstance(T, bool) or isinstance(keep, bool) or not isinstance(T, int) or not isinstance(keep, int) or not 1 <= keep <= T:
            raise ValueError(f"last_frames needs integers 1 <= keep <= T, got T={T!r}, keep={keep!r}")
        return cls.burn_in(T, T - keep, **spec_fields)

    @property
    def base(self) -> LossSpec:
        """The plain LossSpec of the inherited fields."""
        return LossSpec(**{f.name: getattr(self, f.name) for f in dataclasses.fields(LossSpec)})

    @property
    def weighted(self) -> bool:
        return self.frame_weights is not None or self.channel_weights is not None

    @property
    def is_reference(self) -> bool:
        """No weights and every inherited field equals the reference's."""
        return not self.weighted and self.base == _REFERENCE

    def plane_weights(self, T: int, Cy: int) -> list:
        """The table ``q[t * Cy + c] = frame_weights[t] * channel_weights[c]`` as Python floats (f64 products; the caller rounds
        them to f32 once).  ValueError when a tuple's length is not T / Cy."""
        fw, cw = self.frame_weights, self.channel_weights
        if fw is not None and len(fw) != T:
            raise ValueError(f"WeightedLossSpec.frame_weights has {len(fw)} entries, y_pred has T = {T} frames")
        if cw is not None and len(cw) != Cy:
            raise ValueError(f"WeightedLossSpec.channel_weights has {len(cw)} entries, y_pred has Cy = {Cy} channels")
        fw, cw = fw or (1.0,) * T, cw or (1.0,) * Cy
        return [f * c for f in fw for c in cw]


def check_spec(loss, what: str = "loss"):
    """``loss`` keyword of the step / epoch functions: a LossSpec (a WeightedLossSpec is one) or None."""
    if loss is not None and not isinstance(loss, LossSpec):
        raise TypeError(f"{what} must be a LossSpec or None, got {type(loss).__name__}")
    return loss


def compute_loss(y_pred, y, mask=None, use_mask=True, spec=None):
    """Weighted L1 (weight 1+4|y|^3) + 0.005 x spatial-gradient L1; same signature and semantics as
    main.py:28-72.  Inputs are ``[B,T,1,H,W]`` (any leading dims; gradients along the last two).
    ``spec``: a ``LossSpec`` for another point term / weight / gradient coefficient; None and the default spec are the
    reference's loss on the reference's kernels, launch for launch.  A ``WeightedLossSpec`` with weights needs 5-D ``y_pred``
    ``[B,T,Cy,H,W]`` and takes the per-plane-weight entry points; without weights it is its ``base``."""
    check_spec(spec, "spec")
    if isinstance(spec, WeightedLossSpec) and not spec.weighted:
        spec = spec.base
    if spec is not None and spec.is_reference:
        spec = None
    return ops.LossFn.apply(y_pred.contiguous().float(), y, mask, bool(use_mask), spec)
