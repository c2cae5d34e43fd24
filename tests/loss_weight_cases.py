"""f64 restatement of the loss with a weight per plane (unet_convlstm_amd.loss.WeightedLossSpec, include/uclstm.h
uclstm_loss_spec_*_pw), the cases and the inputs of tests/test_loss_weights_host.py and tests/test_gpu_loss_weights.py.

y_pred, y are [B, T, Cy, H, W]; mask the same shape, [B, T, 1, H, W] or None.  With the table
    q[t * Cy + c] = f32(fw[t] * cw[c])            (the product in f64, rounded once; a missing tuple is all ones)
plane p = (b * T + t) * Cy + c has the weight q[p mod (T * Cy)], and with rho, w, m, gd, mc as in loss_spec_cases.py
    s0 = sum(rho w m q), s1 = sum(w m q), s2 = sum(gd mc q), s3 = sum(mc q)
    point = s0 / (s1 + eps) masked,  s0 / (H W B sum(q)) unmasked (m = 1)
    grad  = s2 / (s3 + eps) masked,  s2 / ((H-1) (W-1) B sum(q)) unmasked
    loss  = point + grad_weight * grad; grad_weight == 0: the gradient term does not exist
Every neighbour of the gradient term lies in the element's own plane, so d loss / d y_pred is q_p times the closed form of
loss_spec_cases.loss_bwd_ref.  The references use the f32-rounded table, as the kernels read it.

Rounding (counted, not measured): the kernels multiply each term of a sum, and each gradient element, by q once more in f32 than
the plain kernels do, so the counts of loss_spec_cases.py grow by one: power + 5 per forward term, power + 7 per gradient element.
"""
import dataclasses
import functools

import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when a test file runs as a script)
import boundary_cases as BC
import loss_spec_cases as LC
from unet_convlstm_amd.loss import LossSpec, WeightedLossSpec

F32_UNIT = LC.F32_UNIT

# Distinct entries with a zero and values that are no powers of two, by length.  Cy = 1 runs with channel_weights None: the
# missing tuple that counts as ones.
FRAME_W = {2: (0.0, 1.5), 3: (0.0, 0.25, 1.5), 4: (0.7, 0.0, 0.25, 1.5)}
CHANNEL_W = {1: None, 3: (1.0, 0.3, 2.0)}

# (B, T, Cy, H, W)
CASES = [
    (2, 3, 1, 7, 1),        # a one-column plane: no cells, so only specs without the gradient term; Cy = 1, frame weights alone
    (2, 2, 3, 3, 5),        # H*W = 15, 180 elements: without the gradient term V = 4 groups straddle planes, each element its own q
    (2, 3, 3, 8, 8),        # V = 4 with the gradient term; the broadcast mask at Cy = 3
    (2, 3, 3, 5, 7),        # V = 1 with the gradient term (and without: 630 elements)
    (1, 4, 3, 256, 256),    # V = 4 and more than one trip of the grid-stride loop
    (1, 4, 3, 256, 257),    # V = 1 (with the gradient term) and more than one trip of the grid-stride loop
]
LARGE_CASES = CASES[4:]
SMALL_CASES = CASES[:4]
NOGRAD_SPECS = tuple(n for n, s in LC.SPECS.items() if s.grad_weight == 0)
MASKS = ("none", "plane", "broadcast")      # mask NULL / a mask plane per plane (mask_div 1) / [B,T,1,H,W] (mask_div Cy)


def flat(case):
    """(planes, H, W) of a case."""
    B, T, Cy, H, W = case
    return (B * T * Cy, H, W)


def spec_for(name, case, weights=True):
    """LC.SPECS[name] with the weight tuples of the case's T and Cy (weights False: with both tuples None)."""
    _, T, Cy, _, _ = case
    fields = dataclasses.asdict(LC.SPECS[name])
    return WeightedLossSpec(**fields, frame_weights=FRAME_W[T], channel_weights=CHANNEL_W[Cy]) if weights else WeightedLossSpec(**fields)


def runs():
    """(spec name, case, mask kind) of the C ABI tests: every spec on the small cases, LC.LARGE_SPECS (one per point kind and
    gradient flag) on the large ones; the one-column case only without the gradient term; the broadcast mask where Cy > 1."""
    out = []
    for case in CASES:
        names = LC.LARGE_SPECS if case in LARGE_CASES else tuple(LC.SPECS)
        if min(case[3:]) == 1:
            names = NOGRAD_SPECS
        for name in names:
            out += [(name, case, kind) for kind in MASKS if kind != "broadcast" or case[2] > 1]
    return out


@functools.lru_cache(maxsize=None)
def inputs(case, kind):
    """(y_pred, y, mask) as 5-D f32 tensors from boundary_cases.loss_input; mask None, [B,T,Cy,H,W] or [B,T,1,H,W].  Drawn once
    per (case, kind) and shared: treat as read-only."""
    B, T, Cy, H, W = case
    yp, y, mask = BC.loss_input(flat(case), kind == "plane")
    if kind == "broadcast":
        mask = BC.loss_input((B * T, H, W), True)[2].view(B, T, 1, H, W)
    elif mask is not None:
        mask = mask.view(case)
    return yp.view(case), y.view(case), mask


def table(spec, T, Cy):
    """q as f32 [T * Cy]: the f64 products fw[t] * cw[c], rounded to f32 once."""
    fw = spec.frame_weights if spec.frame_weights is not None else (1.0,) * T
    cw = spec.channel_weights if spec.channel_weights is not None else (1.0,) * Cy
    assert len(fw) == T and len(cw) == Cy
    return torch.tensor([float(f) * float(c) for f in fw for c in cw], dtype=torch.float64).float()


def _q5(spec, y):
    _, T, Cy, _, _ = y.shape
    return table(spec, T, Cy).double().view(1, T, Cy, 1, 1)


def n_bwd(spec):
    """f32 roundings of one gradient element: those of loss_spec_cases.n_bwd and the multiplication by q."""
    return spec.weight_power + 7


def fwd_rel_bound(spec, count):
    """Relative bound of each forward sum: non-negative f32 terms of at most power + 5 roundings each (loss_spec_cases' power + 4
    and the multiplication by q), `count` of them added in f64."""
    return (spec.weight_power + 5) * F32_UNIT + count * 2.0 ** -52


def sums_ref(yp, y, mask, spec):
    """The four sums of uclstm_loss_spec_fwd_pw in f64 (mask None: m = 1; a one-channel mask broadcasts) and the number of terms
    of each."""
    yp, y = yp.double(), y.double()
    B, T, Cy, H, W = y.shape
    q = _q5(spec, y)
    m = torch.ones_like(y) if mask is None else mask.double().expand_as(y)
    w = LC._weight(y, spec)
    s = [(LC._rho(yp - y, spec) * w * m * q).sum(), (w * m * q).sum()]
    if spec.grad_weight == 0:
        s += [torch.zeros((), dtype=torch.float64)] * 2
    else:
        mc = m[..., :H - 1, :W - 1]
        s += [(LC._grad_diff(yp, y) * mc * q).sum(), (mc * q).sum()]
    cells = B * T * Cy * (H - 1) * (W - 1)
    return torch.stack(s), (y.numel(), y.numel(), cells, cells)


def denominators(y, mask, use_mask, spec):
    """(d1, d2) in f64: masked s1 + eps and s3 + eps, unmasked H W B sum(q) and (H-1) (W-1) B sum(q)."""
    B, T, Cy, H, W = y.shape
    q = _q5(spec, y)
    if use_mask and mask is not None:
        m = mask.double().expand_as(y)
        return ((LC._weight(y.double(), spec) * m * q).sum() + spec.eps, (m[..., :H - 1, :W - 1] * q).sum() + spec.eps)
    qsum = q.sum()
    return H * W * B * qsum, (H - 1) * (W - 1) * B * qsum


def loss_ref(yp, y, mask, use_mask, spec):
    """The weighted loss in f64, differentiable in yp."""
    yp, y = yp.double(), y.double()
    masked = use_mask and mask is not None
    H, W = y.shape[-2], y.shape[-1]
    q = _q5(spec, y)
    m = mask.double().expand_as(y) if masked else torch.ones_like(y)
    d1, d2 = denominators(y, mask, use_mask, spec)
    point = (LC._rho(yp - y, spec) * LC._weight(y, spec) * m * q).sum() / d1
    if spec.grad_weight == 0:
        return point
    return point + spec.grad_weight * ((LC._grad_diff(yp, y) * m[..., :H - 1, :W - 1] * q).sum() / d2)


def coefs_ref(y, mask, use_mask, spec):
    """(c1, c2) as ops.LossFn forms them for an upstream gradient of 1: the reciprocal denominators, grad_weight in c2."""
    d1, d2 = denominators(y, mask, use_mask, spec)
    return 1.0 / float(d1), (spec.grad_weight / float(d2) if spec.grad_weight != 0 else 0.0)


def loss_bwd_ref(yp, y, mask, spec, c1, c2):
    """(grad, mag) in f64, [B,T,Cy,H,W]: q_p times loss_spec_cases.loss_bwd_ref on the planes, the mask expanded over channels."""
    B, T, Cy, H, W = y.shape
    m = None if mask is None else mask.expand_as(y).reshape(-1, H, W)
    grad, mag = LC.loss_bwd_ref(yp.reshape(-1, H, W), y.reshape(-1, H, W), m, spec, c1, c2)
    q = _q5(spec, y)
    return grad.view(y.shape) * q, mag.view(y.shape) * q


def vectorised(name, case):
    return LC.vectorised(LC.SPECS[name], flat(case))


# ---------------------------------------------------------------------------------------------
# which instance each case reaches (loss_spec_vec and load_plane_w in csrc/loss_optim.hip)
# ---------------------------------------------------------------------------------------------
NT = LC.NT
# the one-column plane: V = 1 (42 elements), and no spec with the gradient term runs on it
assert not vectorised("l1_nograd", CASES[0]) and all(n in NOGRAD_SPECS for n, c, _ in runs() if c == CASES[0])
# 180 elements in planes of 15: V = 4 without the gradient term, and a group of four straddles two planes; V = 1 with it
assert vectorised("l1_nograd", CASES[1]) and (CASES[1][3] * CASES[1][4]) % 4 != 0 and not vectorised("reference", CASES[1])
# 8 x 8: V = 4 with and without the gradient term, groups inside one plane
assert vectorised("reference", CASES[2]) and vectorised("l1_nograd", CASES[2]) and (8 * 8) % 4 == 0
# 5 x 7: V = 1 with and without the gradient term
assert not vectorised("reference", CASES[3]) and not vectorised("l1_nograd", CASES[3])
# the large cases: V = 4 / V = 1 (with the gradient term) through more than one trip of the grid-stride loop of either kernel
assert all(vectorised(n, CASES[4]) for n in LC.LARGE_SPECS) and 12 * 256 * 256 // 4 > NT * LC.V4_GRID_CAP
assert not vectorised("reference", CASES[5]) and 12 * 256 * 257 > NT * max(LC.FWD_GRID_CAP, LC.BWD_GRID_CAP)
assert {(LC.SPECS[n].point, LC.SPECS[n].grad_weight != 0) for n in LC.LARGE_SPECS} == {("l1", True), ("l2", False), ("huber", True), ("huber", False)}
# every weight tuple has a zero, distinct entries and an entry that is no power of two; the tables have distinct positive entries
for _w in list(FRAME_W.values()) + [CHANNEL_W[3]]:
    assert len(set(_w)) == len(_w) and any(torch.tensor(v).frexp()[0] != 0.5 for v in _w if v > 0)
assert all(0.0 in _w for _w in FRAME_W.values())
for _case in CASES:
    _t = table(spec_for("reference", _case), _case[1], _case[2])
    _pos = _t[_t > 0]
    assert len(_pos) >= 2 and len(set(_pos.tolist())) == len(_pos) and bool((_t == 0).any()), _case
