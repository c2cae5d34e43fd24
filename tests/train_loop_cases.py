"""Helpers of the multi-step training-loop tests that need no GPU (tests/test_train_loop_host.py checks them on the CPU,
tests/test_gpu_train_loop.py uses them on the device).

From the second step on a training step depends on host state that survives from one step to the next: the look-ahead packing
plan of ``ops.prepack_begin`` / ``pack_weights`` (a panel is keyed by the weight's address, not by its contents), the persistent
``_PackBatch`` and the optimiser's raw-pointer updates.  The helpers here are

  * ``oracle_trajectory``: the CPU oracle (oracle/unet_oracle.py) trained for several steps on one batch, every step's snapshot,
    prediction and gradients kept -- the yardstick of "each step against the oracle from the device's own state", and of the
    negative control: a forward pass on the PREVIOUS step's weights must be told apart from one on the live weights;
  * ``PackSpy``: a counting wrapper for ``ops.pack_weights`` that knows, before the call, whether it will be served from the
    look-ahead panels;
  * ``first_difference`` / ``compare``: bit-exact comparison of two snapshots of a run, naming the first tensor that differs.
"""
import ctypes as C

import torch

from conftest import rel_l2
from oracle import unet_oracle as O

LR, WD, CLIP, STEPS = 3e-3, 1e-4, 1.0, 4          # of every multi-step test unless it says otherwise
ORACLE_STEPS = 3
PER_T_BOUND, LOSS_BOUND = 1.5e-2, 2e-3           # tests/test_gpu_model.py: train forward / loss against the bf16-storage oracle
STALE_MIN = 4 * PER_T_BOUND                       # a forward pass on weights that are one step old must be at least this far away
FLAT_KEYS = ("flat_g", "flat_p", "m", "v")


# ---------------------------------------------------------------------------------------------
# the oracle's own trajectory
# ---------------------------------------------------------------------------------------------
def oracle_trajectory(p, x, y, mask, steps=ORACLE_STEPS, lr=LR, wd=WD, use_mask=True):
    """``steps`` optimisation steps of the f32 oracle on one batch.  Entry k (0-based) holds what step k + 1 started from
    (``snapshot``), what it computed (``loss``, ``y_pred``, ``grads`` before the clip) and what it left (``after``)."""
    out, m, v = [], None, None
    p = {k: t.detach().clone() for k, t in p.items()}
    for k in range(steps):
        loss, after, grads, m, v, y_pred = O.train_step(p, x, y, mask, use_mask, m, v, k + 1, lr=lr, wd=wd)
        out.append(dict(snapshot=p, loss=loss, y_pred=y_pred, grads=grads, after=after))
        p = after
    return out


def per_t(got, ref):
    return [rel_l2(got[:, t], ref[:, t]) for t in range(ref.shape[1])]


def stale_distances(preds_fresh, preds_stale):
    """Per-timestep rel-L2 of step k's prediction against the prediction from the weights of step k - 1, for k = 2 .. (1-based):
    ``preds_fresh[k]`` against ``preds_stale[k - 1]``.  The batch is the same at every step, so the forward pass on the previous
    snapshot IS the previous step's reference prediction."""
    return [per_t(preds_fresh[k], preds_stale[k - 1]) for k in range(1, len(preds_fresh))]


# ---------------------------------------------------------------------------------------------
# counting wrapper of ops.pack_weights
# ---------------------------------------------------------------------------------------------
class PackSpy:
    """Stands in for ``ops.pack_weights`` (``monkeypatch.setattr(ops, "pack_weights", spy)``).  ``calls``: one
    ``(step, lookahead, hit, key)`` per call, ``hit`` = the look-ahead state hands out a panel packed at the start of the step
    (decided from the module's state BEFORE the call, by the rule of ``pack_weights`` itself).  ``keep_panels``: ``panels`` gets
    ``(step, descriptor copy, weight, elem_offset, dtype, returned panel)`` for every hit.  ``step`` is set by the caller."""

    def __init__(self, ops, keep_panels=False):
        self.ops, self.real, self.keep_panels = ops, ops.pack_weights, keep_panels
        self.calls, self.panels, self.step = [], [], 0

    def __call__(self, desc, w, elem_offset=0, dtype=None, lookahead=True):
        ops = self.ops
        dtype = ops.BF16 if dtype is None else dtype
        key = (w.data_ptr(), elem_offset, bytes(desc), dtype)
        hit = bool(ops._PACK_RECORDING and lookahead and key in ops._PACK_READY)
        out = self.real(desc, w, elem_offset, dtype, lookahead)
        self.calls.append((self.step, bool(lookahead), hit, key))
        if hit and self.keep_panels:
            d2 = type(desc)()
            C.memmove(C.byref(d2), C.byref(desc), C.sizeof(type(desc)))
            self.panels.append((self.step, d2, w, elem_offset, dtype, out))
        return out

    def of_step(self, step):
        return [c for c in self.calls if c[0] == step]

    def hits(self, step=None):
        return sum(1 for s, _, hit, _ in self.calls if hit and (step is None or s == step))

    def misses(self, step):
        """Calls of ``step`` that asked for a look-ahead panel and were packed in line."""
        return [c for c in self.of_step(step) if c[1] and not c[2]]


# ---------------------------------------------------------------------------------------------
# snapshots of a run, compared bit for bit
# ---------------------------------------------------------------------------------------------
def snapshot(model, opt, loss, **extra):
    """Everything a training step leaves behind, as clones on the tensors' own device: the comparison copies to the host."""
    out = dict(loss=loss.detach().clone(), flat_g=opt.flat.flat_g.clone(), flat_p=opt.flat.flat_p.clone(), m=opt.m.clone(), v=opt.v.clone())
    out.update({"buffer " + k: b.detach().clone() for k, b in model.named_buffers()})
    out.update({k: t.detach().clone() for k, t in extra.items()})
    return out


def layout(model):
    """(names, sizes) of the trainable parameters in the order of the optimiser's flat buffers."""
    named = [(k, p.numel()) for k, p in model.named_parameters() if p.requires_grad]
    return [k for k, _ in named], [n for _, n in named]


_STAGING = [None, None]          # two pinned host buffers, grown on demand: the flat buffers of the base-64 model are 0.4 GB each


def _host(t, slot):
    """``t`` on the host, flat and contiguous.  A large device tensor goes through a pinned buffer that is reused (a fresh
    pageable copy per comparison costs more in page faults than the comparison itself); valid until the slot's next use."""
    t = t.detach().contiguous().view(-1)
    nbytes = t.numel() * t.element_size()
    if not t.is_cuda or nbytes < (1 << 20):
        return t.cpu()
    buf = _STAGING[slot]
    if buf is None or buf.numel() < nbytes:
        buf = _STAGING[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    out = buf[:nbytes].view(t.dtype)
    out.copy_(t)                  # device -> pinned host, synchronous
    return out


def bits_equal(a, b):
    """On the host: same shape, same dtype, same bytes (NaN == NaN, -0.0 != 0.0: ``torch.equal`` on the integer view)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = _host(a, 0), _host(b, 1)
    if a.is_floating_point():
        view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.view(view), b.view(view)
    return torch.equal(a, b)


def first_difference(a, b, names, sizes):
    """(tensor name, rel-L2) of the first tensor in which two snapshots differ, the flat buffers resolved to parameter names
    (as tests/test_gpu_deterministic.py reports it); None when every tensor is bit-identical."""
    if list(a) != list(b):
        return f"keys {sorted(set(a) ^ set(b))[:4]}", float("inf")
    for key in a:
        if bits_equal(a[key], b[key]):
            continue
        x, y = a[key].detach().cpu(), b[key].detach().cpu()
        if key in FLAT_KEYS and x.shape == y.shape and sum(sizes) == x.numel():
            o = 0
            for name, n in zip(names, sizes):
                if not bits_equal(x[o:o + n], y[o:o + n]):
                    return f"{key}[{name}]", rel_l2(x[o:o + n], y[o:o + n])
                o += n
        return key, (rel_l2(x.double(), y.double()) if x.shape == y.shape else float("inf"))
    return None


def compare(what, a, b, names, sizes):
    """Assert that two snapshots are bit-identical; the message names the first differing tensor."""
    diff = first_difference(a, b, names, sizes)
    if diff is not None:
        print(f"[train loop] {what}: first differing tensor {diff[0]}, rel-L2 {diff[1]:.3e}")
    assert diff is None, f"{what}: first differing tensor {diff[0]} (rel-L2 {diff[1]:.3e})"
