"""compute_loss of the reference's main.py:28-72 as one fused HIP reduction (+ one backward kernel), and ``LossSpec``: the same
kernels with the point term (L1 / L2 / Huber), the weight and the gradient term's coefficient as parameters."""
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


def check_spec(loss, what: str = "loss"):
    """``loss`` keyword of the step / epoch functions: a LossSpec or None."""
    if loss is not None and not isinstance(loss, LossSpec):
        raise TypeError(f"{what} must be a LossSpec or None, got {type(loss).__name__}")
    return loss


def compute_loss(y_pred, y, mask=None, use_mask=True, spec=None):
    """Weighted L1 (weight 1+4|y|^3) + 0.005 x spatial-gradient L1; same signature and semantics as
    main.py:28-72.  Inputs are ``[B,T,1,H,W]`` (any leading dims; gradients along the last two).
    ``spec``: a ``LossSpec`` for another point term / weight / gradient coefficient; None and the default spec are the
    reference's loss on the reference's kernels, launch for launch."""
    check_spec(spec, "spec")
    if spec is not None and spec.is_reference:
        spec = None
    return ops.LossFn.apply(y_pred.contiguous().float(), y, mask, bool(use_mask), spec)
