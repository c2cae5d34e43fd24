"""Helpers of tests/test_ema_host.py and tests/test_gpu_ema.py that need no GPU: an f64 restatement of uclstm_ema_update written
from include/uclstm.h, the launch geometry read out of csrc/loss_optim.hip, the error bound and the case lists.

The update (uclstm.h), ema_state = f32[8] {decay, warmup, every, steps_seen, updates_done, reserved x 3}:
    *sumsq given and NaN or infinite       nothing changes: not the shadow, not a count
    otherwise                              steps_seen += 1, and only if (steps_seen + 1) % every == 0 (the OLD count):
        k = updates_done + 1,  d = decay if warmup <= 0 else min(decay, (1 + k) / (warmup + k)), in double, rounded to f32 ONCE
        ema[i] = fma(d, ema[i] - p[i], p[i]);  updates_done += 1

The bound of one update against f64 on the same f32 inputs and the same f32 d, per element:
    |err| <= 3 * 2^-24 * (|ema| + |p|)
u = 2^-24 is the largest relative error of one correctly rounded f32 operation on a NORMAL result.  The subtraction rounds once:
u |ema - p| <= u (|ema| + |p|); the fma rounds once: u |result|, and |result| <= |d| |ema - p| + |p| <= |ema| + |p| (0 < d < 1, the
result is a convex combination); the subtraction's error reaches the result times d < 1.  Together 2u (|ema| + |p|), one unit spare.
The count needs normal results: where BOTH operands are subnormal the result is subnormal too and a correctly rounded f32 is
only within 2^-150 absolute, which no relative bound can ask for.  So the `subnormal` values below pair a subnormal with a normal
number, or with itself (an exact result), and `both_subnormal` is checked for something stronger instead: every f64 intermediate
is then exact (multiples of 2^-173 below 2^-125 fit 53 bits), so the device result must equal the f64 result rounded to f32 BIT
FOR BIT -- which also shows that subnormals are not flushed.
"""
import os
import re

import numpy as np

U32 = 2.0 ** -24
BOUND_UNITS = 3.0
F64_MAX = float(np.finfo(np.float64).max)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "unet-convlstm_amd", "csrc", "loss_optim.hip")

STATE_LEN = 8
I_DECAY, I_WARMUP, I_EVERY, I_SEEN, I_DONE = range(5)


# ---------------------------------------------------------------------------------------------
# launch geometry, from the code
# ---------------------------------------------------------------------------------------------
def kernel_constants(path: str = SOURCE) -> dict:
    """NT (threads per block), U (loads in flight per lane) and the grid cap of the EMA sweep and the swap, read out of the source."""
    with open(path) as f:
        text = f.read()
    out = {}
    for key, name in (("NT", "NT"), ("U", "EMA_U"), ("GRID_CAP", "EMA_GRID_CAP")):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"constexpr int {name} not found in {path}"
        out[key] = int(m.group(1))
    # the launches must really use them: grid_for((n + EMA_U - 1) / EMA_U, EMA_GRID_CAP) blocks of NT threads, twice
    assert len(re.findall(r"grid_for\(\(n \+ EMA_U - 1\) / EMA_U, EMA_GRID_CAP\)\), dim3\(NT\)", text)) == 2
    return out


def grid_blocks(n: int, c: dict) -> int:
    """grid_for((n + U - 1) / U, GRID_CAP): ceil over NT, capped, at least 1."""
    items = (n + c["U"] - 1) // c["U"]
    return max(1, min((items + c["NT"] - 1) // c["NT"], c["GRID_CAP"]))


def abi_sizes(c: dict) -> list:
    """1, NT - 1, NT, one full chunk, a full chunk plus a partial one in a second block, and the smallest n at which a block makes
    a second grid-stride trip, which is then the partial last chunk (one element past GRID_CAP full chunks)."""
    nt, u, cap = c["NT"], c["U"], c["GRID_CAP"]
    return [1, nt - 1, nt, u * nt, u * nt + 3, cap * u * nt + 1]


def trips_of_block0(n: int, c: dict) -> int:
    chunk = c["U"] * c["NT"]
    chunks = (n + chunk - 1) // chunk
    g = grid_blocks(n, c)
    return (chunks + g - 1) // g


# ---------------------------------------------------------------------------------------------
# the f64 restatement
# ---------------------------------------------------------------------------------------------
def overflowed(ss: float) -> bool:
    """step_overflowed of the optimiser kernels: NaN or infinite."""
    return not (abs(float(ss)) <= F64_MAX)


def make_state(decay: float, warmup: float, every: int, seen: int = 0, done: int = 0) -> np.ndarray:
    s = np.zeros(STATE_LEN, dtype=np.float32)
    s[I_DECAY], s[I_WARMUP], s[I_EVERY], s[I_SEEN], s[I_DONE] = decay, warmup, every, seen, done
    return s


def decay_of(state: np.ndarray) -> np.float32:
    """The f32 decay of the NEXT update, from the f32 state: double arithmetic, one rounding."""
    decay, warmup, k = float(state[I_DECAY]), float(state[I_WARMUP]), float(state[I_DONE]) + 1.0
    return np.float32(min(decay, (1.0 + k) / (warmup + k)) if warmup > 0.0 else decay)


def ema_ref(ema, p, state: np.ndarray, sumsq=None):
    """One call of uclstm_ema_update in f64: ``(new shadow f64, new state f32, d or None)``.  ``ema`` / ``p``: f32 or f64 arrays
    (the f32 inputs of the device, widened); ``d`` is None where the shadow was not updated (a skipped or a not-due step)."""
    e64, p64 = np.asarray(ema, dtype=np.float64), np.asarray(p, dtype=np.float64)
    new = state.copy()
    if sumsq is not None and overflowed(sumsq):
        return e64.copy(), new, None
    due = (float(state[I_SEEN]) + 1.0) % max(float(state[I_EVERY]), 1.0) == 0.0
    new[I_SEEN] = state[I_SEEN] + np.float32(1)
    if not due:
        return e64.copy(), new, None
    d = decay_of(state)
    new[I_DONE] = state[I_DONE] + np.float32(1)
    return float(d) * (e64 - p64) + p64, new, d


def bound(ema, p) -> np.ndarray:
    return BOUND_UNITS * U32 * (np.abs(np.asarray(ema, dtype=np.float64)) + np.abs(np.asarray(p, dtype=np.float64)))


def violations(got, want64, ema, p):
    """``(count of elements outside the bound, worst |err| / bound)``; where the bound is 0 the error must be 0 (ratio inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want64)
    b = bound(ema, p)
    bad = int(np.count_nonzero(~(err <= b)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    return bad, float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------
def _subnormals(rng, n):
    return (rng.integers(1, 1 << 23, n).astype(np.float64) * 2.0 ** -149 * rng.choice([-1.0, 1.0], n)).astype(np.float32)


VALUE_KINDS = ("random", "signed_zero", "subnormal", "equal")


def values(kind: str, n: int, seed: int = 0):
    """``(ema, p)`` f32 arrays of length n."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    if kind == "random":
        return e, p
    if kind == "signed_zero":                       # every combination of +0 / -0 / a number, by position
        z = np.array([0.0, -0.0], dtype=np.float32)
        i = np.arange(n)
        e = np.where(i % 3 == 2, e, z[i % 2])
        p = np.where((i // 3) % 3 == 2, p, z[(i // 3) % 2])
        return e.astype(np.float32), p.astype(np.float32)
    if kind == "subnormal":                         # a subnormal beside a normal number, or beside itself
        s = _subnormals(rng, n)
        i = np.arange(n) % 3
        return np.where(i == 1, e, s).astype(np.float32), np.where(i == 0, p, s).astype(np.float32)
    if kind == "equal":
        return e, e.copy()
    if kind == "both_subnormal":
        return _subnormals(rng, n), _subnormals(rng, n)
    raise ValueError(kind)


# (decay, warmup, every) of the ABI sequences: warm-up on and off, every step and every third
SCHEDULES = [(0.999, 0.0, 1), (0.999, 10.0, 1), (0.9, 0.0, 3), (0.9, 2.0, 3)]

# sumsq of the skip cases: (value, skipped)
SUMSQ_CASES = [(float("inf"), True), (float("nan"), True), (3.5, False)]
