"""f64 restatement of the LossSpec loss (unet_convlstm_amd.loss.LossSpec, include/uclstm.h uclstm_loss_spec_*), the specs and the
inputs of tests/test_loss_spec_host.py and tests/test_gpu_loss_spec.py.

With d = y_pred - y:
    rho(d)  = |d| (l1) / d^2 (l2) / huber: 0.5 d^2 where |d| <= delta, else delta (|d| - 0.5 delta)
    rho'(d) = sign(d) / 2 d / clamp(d, -delta, delta)
    w       = 1 + weight_gain * |y|^weight_power
    point   = sum(rho w m) / (sum(w m) + eps) masked, mean(rho w) unmasked
    grad    = main.py:47-68 unchanged: L1 on the forward differences over the cropped (H-1) x (W-1) cells, the mask at the cell,
              sum / (sum(mc) + eps) masked, a mean unmasked
    loss    = point + grad_weight * grad; grad_weight == 0: the gradient term does not exist

Inputs are boundary_cases.loss_input: multiples of 1/64 in [-4, 4], mask values {0, 1/4, 1/2, 1}, planted exact zeros of d and of
the differences.  d is then a multiple of 1/64 with |d| <= 8: d, d^2 (a multiple of 2^-12 up to 64), 0.5 d^2 and, with delta on the
same grid, delta (|d| - 0.5 delta) are all exact in f32, and so is every comparison of |d| with delta -- no branch of the kernels
depends on their precision.
"""
import functools

import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when a test file runs as a script)
import boundary_cases as BC
from unet_convlstm_amd.loss import LossSpec

F32_UNIT = 2.0 ** -24
NT = BC.NT                                 # csrc/loss_optim.hip: constexpr int NT
FWD_GRID_CAP, BWD_GRID_CAP = 1024, 2048    # blocks of the one-element-per-thread (V = 1) instances, as the reference's kernels
V4_GRID_CAP = 512                          # SPEC_GRID_CAP_V4: blocks of the four-elements-per-thread instances (fwd atomic form, bwd)
DELTAS = (0.5, 2.0)

# (planes, H, W).  The first five are the ones the kernels' paths need from boundary_cases.LOSS_BWD_CASES: a one-column plane,
# 2 x 2, one long odd row, odd sizes over more than one block, and more elements than one trip of the V = 1 grids.  None of them
# has W % 4 == 0, which is what sends a spec WITH the gradient term to the V = 4 instances: (3, 8, 8) of the same list does, and
# (9, 256, 256) is the smallest change of the large case that takes those instances through more than one trip.
CASES = [(2, 7, 1), (3, 2, 2), (1, 3, 341), (5, 17, 19), (9, 256, 257), (3, 8, 8), (9, 256, 256)]
LARGE_CASES = [(9, 256, 257), (9, 256, 256)]
assert all(c in BC.LOSS_BWD_CASES for c in CASES[:6])

SPECS = {
    "reference": LossSpec(),                                   # the reference's parameters, forced through the new kernels
    "masked_mse": LossSpec.masked_mse(),
    "l2_refweight": LossSpec(point="l2"),
    "huber0.5_p1": LossSpec(point="huber", delta=0.5, weight_power=1, weight_gain=2.0),
    "huber2_p1": LossSpec(point="huber", delta=2.0, weight_power=1, weight_gain=0.75, grad_weight=0.02),
    "huber0.5_p2": LossSpec(point="huber", delta=0.5, weight_power=2, weight_gain=1.5, grad_weight=0.02),
    "huber2_p2": LossSpec(point="huber", delta=2.0, weight_power=2, weight_gain=4.0),
    "huber0.5_p4": LossSpec(point="huber", delta=0.5, weight_power=4, weight_gain=0.25),
    "huber2_p4": LossSpec(point="huber", delta=2.0, weight_power=4, weight_gain=1.0, eps=1e-6),
    "l1_nograd": LossSpec(grad_weight=0.0),
    "l2_nograd": LossSpec(point="l2", weight_power=2, weight_gain=3.0, grad_weight=0.0),
    "huber_nograd": LossSpec(point="huber", delta=2.0, grad_weight=0.0),
}
# The large cases are there for the grid-stride loop, which every instance of a kernel shares: they run one spec per combination of
# (gradient term, point kind) instead of all twelve.
LARGE_SPECS = ("reference", "masked_mse", "huber0.5_p4", "huber_nograd")


def runs():
    """(spec name, case, masked) of the C ABI tests."""
    out = []
    for name in SPECS:
        for case in CASES:
            if case in LARGE_CASES and name not in LARGE_SPECS:
                continue
            out += [(name, case, False), (name, case, True)]
    return out


@functools.lru_cache(maxsize=None)
def inputs(case, masked):
    """boundary_cases.loss_input, drawn once per (case, masked) and shared: treat as read-only."""
    return BC.loss_input(case, masked)


def n_bwd(spec):
    """f32 roundings of one gradient element: `power` multiplications and one add for w, three multiplications for the point
    part, one for c2 * gg, the final add."""
    return spec.weight_power + 6


def fwd_rel_bound(spec, count):
    """Relative bound of each forward sum: non-negative f32 terms of at most power + 4 roundings each, `count` of them added in f64."""
    return (spec.weight_power + 4) * F32_UNIT + count * 2.0 ** -52


def _rho(d, spec):
    if spec.point == "l1":
        return d.abs()
    if spec.point == "l2":
        return d * d
    ad = d.abs()
    return torch.where(ad <= spec.delta, 0.5 * d * d, spec.delta * (ad - 0.5 * spec.delta))


def _drho(d, spec):
    if spec.point == "l1":
        return torch.sign(d)
    if spec.point == "l2":
        return 2.0 * d
    return d.clamp(-spec.delta, spec.delta)


def _weight(y, spec):
    return 1.0 + spec.weight_gain * y.abs() ** spec.weight_power


def _grad_diff(yp, y):
    H, W = y.shape[-2], y.shape[-1]
    dxp, dyp = yp[..., :H - 1, 1:] - yp[..., :H - 1, :W - 1], yp[..., 1:, :W - 1] - yp[..., :H - 1, :W - 1]
    dxg, dyg = y[..., :H - 1, 1:] - y[..., :H - 1, :W - 1], y[..., 1:, :W - 1] - y[..., :H - 1, :W - 1]
    return (dxp - dxg).abs() + (dyp - dyg).abs()


def loss_ref(yp, y, mask, use_mask, spec):
    """The loss in f64, differentiable in yp (any leading dimensions; the gradient term along the last two)."""
    yp, y = yp.double(), y.double()
    masked = use_mask and mask is not None
    rw, w = _rho(yp - y, spec) * _weight(y, spec), _weight(y, spec)
    if masked:
        m = mask.double()
        point = (rw * m).sum() / ((w * m).sum() + spec.eps)
    else:
        point = rw.mean()
    if spec.grad_weight == 0:
        return point
    gd = _grad_diff(yp, y)
    if masked:
        mc = m[..., :y.shape[-2] - 1, :y.shape[-1] - 1]
        return point + spec.grad_weight * ((gd * mc).sum() / (mc.sum() + spec.eps))
    return point + spec.grad_weight * gd.mean()


def sums_ref(yp, y, mask, spec):
    """The four sums of uclstm_loss_spec_fwd in f64 (mask None: m = 1) and the number of terms of each."""
    yp, y = yp.double(), y.double()
    m = torch.ones_like(y) if mask is None else mask.double()
    w = _weight(y, spec)
    s = [(_rho(yp - y, spec) * w * m).sum(), (w * m).sum()]
    if spec.grad_weight == 0:
        s += [torch.zeros((), dtype=torch.float64)] * 2
    else:
        mc = m[..., :y.shape[-2] - 1, :y.shape[-1] - 1]
        s += [(_grad_diff(yp, y) * mc).sum(), mc.sum()]
    cells = y.numel() // (y.shape[-2] * y.shape[-1]) * (y.shape[-2] - 1) * (y.shape[-1] - 1)
    return torch.stack(s), (y.numel(), y.numel(), cells, cells)


def coefs_ref(y, mask, use_mask, spec):
    """(c1, c2) as ops.LossFn forms them for an upstream gradient of 1: the reciprocal denominators, grad_weight in c2."""
    y = y.double()
    H, W = y.shape[-2], y.shape[-1]
    cells = y.numel() // (H * W) * (H - 1) * (W - 1)
    if use_mask and mask is not None:
        m = mask.double()
        d1, d2 = float((_weight(y, spec) * m).sum()) + spec.eps, float(m[..., :H - 1, :W - 1].sum()) + spec.eps
    else:
        d1, d2 = float(y.numel()), float(cells)
    return 1.0 / d1, (spec.grad_weight / d2 if spec.grad_weight != 0 else 0.0)


def loss_bwd_ref(yp, y, mask, spec, c1, c2):
    """(grad, mag) in f64 of the closed form of uclstm_loss_spec_bwd on [planes, H, W]:
        grad = c1 * rho'(d) * w * m + c2 * (-(sx + sy) * m + sx(i,j-1) * m(i,j-1) + sy(i-1,j) * m(i-1,j)),
    sx, sy as in boundary_cases.loss_bwd_ref; the second part only with a gradient term (grad_weight != 0);
    mag = |c1| |rho'| w m + |c2| * the sum of the magnitudes of the four gradient terms."""
    a, b = yp.double(), y.double()
    planes, H, W = a.shape
    m = torch.ones_like(a) if mask is None else mask.double()
    d = a - b
    dr, w = _drho(d, spec), _weight(b, spec)
    grad, mag = c1 * dr * w * m, abs(c1) * dr.abs() * w * m
    if spec.grad_weight == 0:
        return grad, mag
    sx, sy = torch.zeros_like(a), torch.zeros_like(a)
    if H > 1 and W > 1:
        sx[:, :H - 1, :W - 1] = torch.sign(d[:, :H - 1, 1:] - d[:, :H - 1, :W - 1])
        sy[:, :H - 1, :W - 1] = torch.sign(d[:, 1:, :W - 1] - d[:, :H - 1, :W - 1])
    gg = -(sx + sy) * m
    gmag = (sx.abs() + sy.abs()) * m
    gg[:, :, 1:] += (sx * m)[:, :, :-1]
    gmag[:, :, 1:] += (sx.abs() * m)[:, :, :-1]
    gg[:, 1:, :] += (sy * m)[:, :-1, :]
    gmag[:, 1:, :] += (sy.abs() * m)[:, :-1, :]
    return grad + c2 * gg, mag + abs(c2) * gmag


def vectorised(spec, case):
    """Whether 16-byte aligned planes of this case take the V = 4 instances (loss_spec_vec in csrc/loss_optim.hip)."""
    planes, H, W = case
    return W % 4 == 0 if spec.grad_weight != 0 else (planes * H * W) % 4 == 0


# ---------------------------------------------------------------------------------------------
# what the cases are there for
# ---------------------------------------------------------------------------------------------
# more than one trip of the grid-stride loop: the V = 1 instances of both kernels on one case, the V = 4 instances on the other
assert not vectorised(SPECS["reference"], LARGE_CASES[0]) and 9 * 256 * 257 > NT * max(FWD_GRID_CAP, BWD_GRID_CAP)
assert vectorised(SPECS["reference"], LARGE_CASES[1]) and 9 * 256 * 256 // 4 > NT * V4_GRID_CAP
assert all(vectorised(SPECS[s], c) and c[0] * c[1] * c[2] // 4 > NT * V4_GRID_CAP for s in ("masked_mse", "huber_nograd") for c in LARGE_CASES)
# both instance widths with and without the gradient term among the small cases
assert {vectorised(SPECS[s], c) for s in ("reference",) for c in CASES[:4] + CASES[5:6]} == {True, False}
assert {vectorised(SPECS[s], c) for s in ("masked_mse",) for c in CASES[:4] + CASES[5:6]} == {True, False}
# |d| < delta, == delta and > delta all occur at either delta (in every case of a thousand elements or more, masked and not)
assert sum(c[0] * c[1] * c[2] >= 1000 for c in CASES) == 4
for _case in [c for c in CASES if c[0] * c[1] * c[2] >= 1000]:
    for _masked in (False, True):
        _ad = (inputs(_case, _masked)[0] - inputs(_case, _masked)[1]).abs()
        for _delta in DELTAS:
            assert bool((_ad < _delta).any()) and bool((_ad == _delta).any()) and bool((_ad > _delta).any()), (_case, _masked, _delta)
        assert bool((_ad == 0).any())
assert {s.delta for s in SPECS.values() if s.point == "huber"} == set(DELTAS)
assert {(s.point, s.weight_power) for s in SPECS.values() if s.point == "huber" and s.grad_weight != 0} == {("huber", p) for p in (1, 2, 4)}
assert {s.point for s in SPECS.values() if s.grad_weight == 0} == {"l1", "l2", "huber"}
