"""Helpers of tests/test_monitor_host.py and tests/test_gpu_monitor.py that need no GPU: an f64 restatement of uclstm_param_stats
written from include/uclstm.h (the eight columns of one tensor, and one whole call: blocks, ring slot, meta row, counters), the
error bound of the three sums, and the case generators the two files share.

One call (uclstm.h), state = int64[8] {every, steps_seen, records_done, due, slot, reserved x 3}:
    steps_seen += 1;  due = steps_seen % every == 0;  slot = records_done % history   (due and slot are left in the state)
    not due: nothing else changes, prev included
    due: ring[slot][t] = the eight columns of tensor t, meta[slot] = {steps_seen, scale or 1, sumsq or NaN, skipped},
         prev = p (where prev is given), records_done += 1
Columns, over the elements of a tensor, everything widened to f64:
    0 sum g^2 over finite g   1 max |g| over finite g (0: none)   2 non-finite g   3 g == 0 (+0 and -0)
    4 sum p^2 over finite p   5 max |p| over finite p             6 non-finite p   7 sum (p - prev)^2, both finite (0: no prev)

The bound of a sum against this restatement: |dev - ref| <= (count + 4) * 2^-53 * ref, count = the tensor's elements.  Every term
is a non-negative f64: g^2 and p^2 are exact products of f32 values (48 significant bits), so any order of adding `count` of them
stays within (count - 1) * 2^-53 relative of the exact sum, and the restatement adds with math.fsum (the exact sum, rounded
once); the difference p - prev and its square round
once each, identically on both sides (no fused multiply-add on either), which the spare units cover with room.
"""
import math

import numpy as np

from unet_convlstm_amd import _lib as L
from unet_convlstm_amd.optim import build_stat_blocks

COLS = 8
SUM_COLS = (0, 4, 7)
MAX_COLS = (1, 5)
COUNT_COLS = (2, 3, 6)
STATE_LEN = 8
I_EVERY, I_SEEN, I_DONE, I_DUE, I_SLOT = range(5)
F64_MAX = float(np.finfo(np.float64).max)
U64 = 2.0 ** -53


def chunk() -> int:
    """Elements one block reduces: asked of the library (a host function, no launch)."""
    return int(L.lib.uclstm_param_stats_chunk())


def abi_sizes(c: int) -> list:
    """The sizes the issue lists: one element, one short of a block, a block, one over, three blocks and a ragged rest."""
    return [1, c - 1, c, c + 1, 3 * c + 5]


def abi_layout(c: int) -> list:
    """Those sizes laid end to end so that tensors start at element offsets 0, 1, 2 and 3 mod 4 (c is a multiple of 4), plus a
    short last tensor that the value generator fills with NaN."""
    return [1, c + 1, c - 1, 1, 3 * c + 5, c, 1, c + 1, 1, 7]


def offsets_of(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)


# ---------------------------------------------------------------------------------------------
# the f64 restatement
# ---------------------------------------------------------------------------------------------
def overflowed(ss: float) -> bool:
    """step_overflowed of the optimiser kernels: NaN or infinite."""
    return not (abs(float(ss)) <= F64_MAX)


def tensor_ref(g, p, prev=None) -> np.ndarray:
    """The eight columns of one tensor from its f32 elements, in f64."""
    g32, p32 = np.asarray(g, dtype=np.float32), np.asarray(p, dtype=np.float32)
    g64, p64 = g32.astype(np.float64), p32.astype(np.float64)
    gf, pf = np.isfinite(g64), np.isfinite(p64)
    out = np.zeros(COLS, dtype=np.float64)
    out[0] = math.fsum(np.square(g64[gf]).tolist())
    out[1] = np.max(np.abs(g64[gf]), initial=0.0)
    out[2] = np.count_nonzero(~gf)
    out[3] = np.count_nonzero(g64 == 0.0)
    out[4] = math.fsum(np.square(p64[pf]).tolist())
    out[5] = np.max(np.abs(p64[pf]), initial=0.0)
    out[6] = np.count_nonzero(~pf)
    if prev is not None:
        q64 = np.asarray(prev, dtype=np.float32).astype(np.float64)
        both = pf & np.isfinite(q64)
        d = p64[both] - q64[both]
        out[7] = math.fsum((d * d).tolist())
    return out


def make_state(every: int, seen: int = 0, done: int = 0) -> np.ndarray:
    s = np.zeros(STATE_LEN, dtype=np.int64)
    s[I_EVERY], s[I_SEEN], s[I_DONE] = every, seen, done
    return s


def call_ref(p, g, prev, sizes, ring, meta, state, history, sumsq=None, scale=None):
    """One call in f64: ``(ring, meta, state, prev, recorded)``, all new arrays.  ``prev`` None: no update column, nothing rewritten."""
    ring, meta, state = np.array(ring, dtype=np.float64), np.array(meta, dtype=np.float64), np.array(state, dtype=np.int64)
    new_prev = None if prev is None else np.array(prev, dtype=np.float32)
    seen = int(state[I_SEEN]) + 1
    due = seen % max(int(state[I_EVERY]), 1) == 0
    slot = int(state[I_DONE]) % history
    state[I_SEEN], state[I_DUE], state[I_SLOT] = seen, int(due), slot
    if not due:
        return ring, meta, state, new_prev, False
    for t, (o, n) in enumerate(zip(offsets_of(sizes), sizes)):
        ring[slot, t] = tensor_ref(g[o:o + n], p[o:o + n], None if prev is None else prev[o:o + n])
    meta[slot] = [float(seen), 1.0 if scale is None else float(np.float32(scale)), np.nan if sumsq is None else float(sumsq),
                  1.0 if (sumsq is not None and overflowed(sumsq)) else 0.0]
    state[I_DONE] += 1
    if prev is not None:
        new_prev = np.array(p, dtype=np.float32)
    return ring, meta, state, new_prev, True


def compare_rows(got, want, sizes):
    """Device rows f64 [n, 8] against the restatement's: ``(mismatches, over_half)``.  Counts and maxima must be equal, a sum
    within (count + 4) * 2^-53 * ref; ``mismatches`` lists ``(tensor, column, got, want)``, ``over_half`` counts the tensors in which
    a sum spends more than half of its bound."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == (len(sizes), COLS), (got.shape, want.shape)
    bad, over_half = [], 0
    for t, n in enumerate(sizes):
        for c in MAX_COLS + COUNT_COLS:
            if not got[t, c] == want[t, c]:
                bad.append((t, c, got[t, c], want[t, c]))
        half = False
        for c in SUM_COLS:
            b = (int(n) + 4) * U64 * want[t, c]
            err = abs(got[t, c] - want[t, c])
            if not err <= b:
                bad.append((t, c, got[t, c], want[t, c]))
            half |= err > 0.5 * b
        over_half += int(half)
    return bad, over_half


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
_SUB = np.float32(2.0 ** -140)
SPECIALS = [np.float32(0.0), np.float32(-0.0), _SUB, -_SUB, np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), None]


def planted(sizes, c: int, seed: int = 0, nan_tensor=None):
    """``(g, p, prev)`` f32 arrays over the layout: random numbers, with +-0, subnormals, +-inf and NaN planted at the first and the
    last element of blocks (the next value of SPECIALS from block to block, None leaving the element alone), and a few in the middle; ``prev`` is
    ``p`` moved a little, with non-finite values of its own.  Tensor ``nan_tensor`` is NaN in all three."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    prev = (p.astype(np.float64) + rng.standard_normal(n) * 1e-3).astype(np.float32)
    blocks, _ = build_stat_blocks(sizes, c)
    k = len(SPECIALS)
    big = 0                                          # blocks of more than one element, counted: their last element is an edge of its own
    for b, (_, start, count) in enumerate(blocks.tolist()):
        for arr, shift in ((g, 0), (p, 2), (prev, 5)):
            first, last = SPECIALS[(b + shift) % k], SPECIALS[(big + shift + 4) % k]
            if first is not None:
                arr[start] = first
            if last is not None and count > 1:
                arr[start + count - 1] = last
        big += count > 1
    for arr in (g, p, prev):
        mid = rng.integers(0, n, 3 * k)
        for j, i in enumerate(mid.tolist()):
            if SPECIALS[j % k] is not None:
                arr[i] = SPECIALS[j % k]
    if nan_tensor is not None:
        o = int(offsets_of(sizes)[nan_tensor])
        for arr in (g, p, prev):
            arr[o:o + sizes[nan_tensor]] = np.nan
    return g, p, prev


# sumsq / scale of the meta cases: (sumsq, scale, skipped)
META_CASES = [(None, None, False), (3.5, None, False), (float("inf"), 1024.0, True), (float("nan"), 0.5, True), (F64_MAX, 65536.0, False)]
