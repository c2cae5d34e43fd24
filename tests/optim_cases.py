"""Helpers of tests/test_gpu_optim_abi.py and tests/test_optim_cases_host.py that need no GPU: f64 references of the optimiser
family of csrc/loss_optim.hip (uclstm_adamw_step, _step_dev, _step_scaled, _step_groups, uclstm_loss_scale_update), written from
include/uclstm.h and nothing else, the counted error bounds, the case tables and the input generators.
tests/test_optim_cases_host.py pins every reference to torch.optim.AdamW in f64 on the CPU, shows that a plain f32 evaluation of
the header's formulas lies inside every bound, and that six wrong ones do not.

The update (uclstm.h; main.py:106-108, 275), per element, all hyper-parameters f32 values:
    gi  = g * coef                       coef = min(1, max_norm / (sqrt(*sumsq) + float32(1e-6))), or 1 without clipping;
                                         the scaled forms: (1 / scale) * min(1, max_norm / (sqrt(*sumsq) / scale + float32(1e-6)))
    m'  = b1 * m + (1 - b1) * gi
    v'  = b2 * v + (1 - b2) * gi * gi
    p'  = (1 - lr * wd) * p - (lr / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps),        bc = 1 - beta^step

Bounds are COUNTED, not measured.  u = 2^-24 is the largest relative error of one correctly rounded f32 operation.  The library
is built without any fast-math flag (build.py FLAGS: -O3 -std=c++17 -fPIC -fno-gpu-rdc, nothing else that touches arithmetic), so
sqrtf and / are the correctly rounded forms and count u like *, + and fma.  Every f32 operation of the kernels contributes u times
the magnitude of its own result, propagated to first order through the f64 formula; a fused multiply-add has one rounding where
the separate forms have two, so the count below (no fusion) covers every contraction the compiler may choose.

  clip coefficient (relative, `coef_rel`):
      not clipped (no sumsq, max_norm <= 0), or the f64 quotient above 1 by more than 8u: the f32 coefficient is exactly 1     0
      plain:   (float)sqrt(*sumsq) u,  + 1e-6f u,  max_norm / . u                                                             3u
      scaled:  inv_scale = 1 / scale u; no clipping: coef = inv_scale                                                          u
               clipping: (float)sqrt u, * inv_scale (its own rounding u, and inv_scale's u), + 1e-6f u, / u  = 5u for the
               factor (0 where it is exactly 1), coef = inv_scale * factor: inv_scale's u and the product's u                 7u
  gi: e_g = coef_rel + u (the product; 0 when coef is exactly 1 and exact)
  m': b1*m u|t1|;  1-b1 u, its product with gi u, gi itself e_g: (2u + e_g)|t2|;  the sum u(|t1| + |t2|)
          bound_m = 2u |b1 m| + (3u + e_g) |(1-b1) gi|            -- the scale is the two terms' magnitudes, they can cancel
  v': b2*v u s1;  1-b2 u, two products 2u, gi twice 2 e_g: (3u + 2 e_g) s2;  the sum u (s1 + s2)
          bound_v = 2u b2 v + (4u + 2 e_g) (1-b2) gi^2
  bias corrections: pow, 1 - . and 1 / . (1 / sqrt .) in double, then ONE rounding to f32: u + 2^-50 / bc (the double part)
  denom = sqrtf(v') * inv_sqrt_bc2 + eps:  A = sqrt(v')/sqrt(bc2) carries sqrtf u, half of v''s relative error bound_v / v',
          inv_sqrt_bc2 u + 2^-50/bc2, the product u;  the sum u * denom:       err_denom = A (3u + bound_v/(2 v') + 2^-50/bc2) + u denom
  update U = (lr * inv_bc1) * m' / denom:  inv_bc1 u + 2^-50/bc1, lr * . u, * m' u, / denom u, m' itself bound_m, denom itself:
          err_U = |U| (4u + 2^-50/bc1 + err_denom / denom) + bound_m * lr / (bc1 denom)
  decay * p:  decay = 1 - lr*wd: the product u |lr wd|, the difference u |decay|;  decay * p u:
          err_dp = (u (|lr wd| + |decay|) / |decay| + u) |decay p|         (3u |decay p| up to lr wd)
  p' = decay*p - U:  u |p'|  + err_dp + err_U
All three bounds are multiplied by 1 + 2^-10 for the second-order terms a first-order count leaves out.  No constant here comes
from what a kernel produced.  The inputs keep every non-zero g*coef at or above 2^-60 in magnitude, so that gi*gi and the terms of
v' stay normal f32 numbers and u stays a relative error (asserted in adamw_ref).
"""
import math

import numpy as np

U32 = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -10
F32_1EM6 = float(np.float32(1e-6))

# launch geometry mirrored from csrc/loss_optim.hip (a case that is meant to reach a path asserts against these)
NT = 256                                  # constexpr int NT
GRID_CAP = 2048                           # grid_for(n, 2048) of the single-group kernels, grid_for((n + 3) / 4, 2048) of the groups kernel
SWEEP = NT * GRID_CAP                     # elements of one trip of `i += gridDim.x * NT`: 524 288
CHUNK = 4 * NT                            # adamw_groups_kernel: U * NT elements per block iteration, lane t takes t, 256 + t, 512 + t, 768 + t
GROUPS_SWEEP = CHUNK * GRID_CAP           # 2 097 152: where a block's second trip begins
LDS_FILL = NT                             # `for (k = threadIdx.x; k < n_groups; k += NT)`: a second trip above 256 groups
MAX_GROUPS = 1024


def f32(x):
    return float(np.float32(x))


# (lr, beta1, beta2, eps, weight_decay) as f32 values.  Group k of a run-table case uses set k % 8.
HYPER_SETS = [tuple(f32(x) for x in h) for h in (
    (1e-3, 0.9, 0.999, 1e-8, 1e-4),       # 0: the model's own (main.py:275)
    (1e-3, 0.9, 0.999, 1e-8, 0.0),        # 1: no weight decay
    (1e-3, 0.0, 0.999, 1e-8, 1e-4),       # 2: beta1 = 0: bc1 == 1, m' = g
    (0.0, 0.9, 0.999, 1e-8, 1e-4),        # 3: lr = 0: only m, v move, p bit-identical
    (1e-2, 0.8, 0.99, 1e-6, 1e-2),
    (3e-4, 0.95, 0.98, 1e-8, 0.1),
    (1e-3, 0.5, 0.9, 1e-3, 0.0),          # 6: eps dominates the denominator
    (5e-2, 0.9, 0.999, 1e-8, 1e-2),
)]
HYPER_MODEL, HYPER_WD0, HYPER_B1_0, HYPER_LR0 = 0, 1, 2, 3
STEPS = (1, 2, 3, 4, 10, 1000)
BIG_STEP = 100000                         # 0.9^t underflows to 0 in double, 0.999^t = 3.5e-44 < 2^-53: both bc == 1 exactly
SCALES = (1.0, 1024.0, 2.0 ** 24)

# (name, *sumsq or None for a NULL pointer, max_norm): *sumsq is a chosen f64 value, never uclstm_sumsq's
CLIP_CASES = [
    ("null", None, 1.0),
    ("max_norm_0", 4.0, 0.0),
    ("max_norm_neg", 4.0, -1.0),
    ("below", 0.25, 1.0),                 # norm 0.5 < max_norm: the coefficient is exactly 1
    ("x50", 2500.0, 1.0),                 # norm 50 x max_norm
    ("zero", 0.0, 1.0),
]
CLIP_X50 = CLIP_CASES[4]

SINGLE_N = (1, 255, 256, 257, SWEEP + 257)
assert SINGLE_N[-1] > SWEEP and (SINGLE_N[-1] - SWEEP) % NT != 0          # second trip, and a ragged last block on it


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def clip_coef_ref(sumsq, max_norm, scale=None):
    """(coef, coef_rel): the f64 coefficient g is multiplied by, and the counted relative error of its f32 evaluation."""
    clip = sumsq is not None and max_norm > 0
    inv = 1.0 if scale is None else 1.0 / float(scale)
    if not clip:
        return inv, (0.0 if scale is None else U32)
    q = float(max_norm) / (math.sqrt(float(sumsq)) * inv + F32_1EM6)
    factor_exact = q > 1.0 + 8 * U32                         # then the f32 quotient is above 1 too and fminf returns 1
    if scale is None:
        return min(1.0, q), (0.0 if factor_exact else 3 * U32)
    return inv * min(1.0, q), (U32 if factor_exact else 7 * U32)


def adamw_ref(p, m, v, g, coef, lr, b1, b2, eps, wd, step, coef_rel=0.0):
    """One step in f64 from the f32 inputs.  Hyper-parameters are scalars or per-element arrays.  Returns p', m', v' and the
    counted bounds bound_p, bound_m, bound_v (module docstring)."""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    lr, b1, b2, eps, wd = (np.asarray(a, dtype=np.float64) for a in (lr, b1, b2, eps, wd))
    u = U32
    gi = g * coef
    assert bool(np.all((gi == 0) | (np.abs(gi) >= 2.0 ** -60))), "inputs: a non-zero g * coef below 2^-60"
    e_g = 0.0 if (coef == 1.0 and coef_rel == 0.0) else coef_rel + u
    t1, t2 = b1 * m, (1.0 - b1) * gi
    m2 = t1 + t2
    bm = 2 * u * np.abs(t1) + (3 * u + e_g) * np.abs(t2)
    s1, s2 = b2 * v, (1.0 - b2) * gi * gi
    v2 = s1 + s2
    bv = 2 * u * s1 + (4 * u + 2 * e_g) * s2
    with np.errstate(under="ignore"):
        bc1, bc2 = 1.0 - np.power(b1, float(step)), 1.0 - np.power(b2, float(step))
    A = np.sqrt(v2) / np.sqrt(bc2)
    denom = A + eps
    ev = np.divide(bv, v2, out=np.zeros_like(v2), where=v2 > 0)
    b_denom = A * (3 * u + 0.5 * ev + 2.0 ** -50 / bc2) + u * denom
    k = lr / bc1 / denom
    upd = k * m2
    b_upd = np.abs(upd) * (4 * u + 2.0 ** -50 / bc1 + b_denom / denom) + bm * np.abs(k)
    decay = 1.0 - lr * wd
    dp = decay * p
    b_dp = (u * (np.abs(lr * wd) + np.abs(decay)) / np.abs(decay) + u) * np.abs(dp)
    p2 = dp - upd
    bp = u * np.abs(p2) + b_dp + b_upd
    return p2, m2, v2, bp * SECOND_ORDER, bm * SECOND_ORDER, bv * SECOND_ORDER


def group_index(runs, n):
    """The group of every element, from a run table i64 [n_runs][3] {begin, end, group}."""
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 3)
    return np.repeat(runs[:, 2], runs[:, 1] - runs[:, 0])[:n].copy()


def group_hypers(grp, n_groups):
    """Per-element (lr, b1, b2, eps, wd): group k uses HYPER_SETS[k % 8]."""
    table = np.array([HYPER_SETS[k % 8] for k in range(n_groups)], dtype=np.float64)
    return tuple(table[grp, j] for j in range(5))


def groups_ref(p, m, v, g, coef, runs, n_groups, step, coef_rel=0.0):
    """adamw_ref per element, the element's hyper-parameters taken from its group."""
    grp = group_index(runs, len(p))
    assert len(grp) == len(p)
    return adamw_ref(p, m, v, g, coef, *group_hypers(grp, n_groups), step, coef_rel)


def step_overflowed(sumsq):
    """The header's overflowed step: *sumsq NaN or infinite."""
    return not math.isfinite(float(sumsq))


def loss_scale_update_ref(state, sumsq, growth, backoff, interval):
    """The exact next f32 state {scale, growth tracker, successful steps} (uclstm.h)."""
    F = np.float32
    s = [F(x) for x in state]
    if step_overflowed(sumsq):
        s[0] = max(F(s[0] * F(backoff)), F(1.0))
        s[1] = F(0.0)
    else:
        s[2] = F(s[2] + F(1.0))
        s[1] = F(s[1] + F(1.0))
        if s[1] >= F(interval):
            s[0] = min(F(s[0] * F(growth)), F(16777216.0))
            s[1] = F(0.0)
    return [float(x) for x in s]


# The transitions of uclstm_loss_scale_update, written by hand (tests/test_optim_cases_host.py holds loss_scale_update_ref to them,
# tests/test_gpu_optim_abi.py the device).
# (state, *sumsq, growth, backoff, interval) -> next state, written by hand
INF, NAN = float("inf"), float("nan")
LOSS_SCALE_TABLE = [
    ([1024.0, 0.0, 0.0], 1.0, 2.0, 0.5, 3, [1024.0, 1.0, 1.0]),
    ([1024.0, 1.0, 1.0], 0.0, 2.0, 0.5, 3, [1024.0, 2.0, 2.0]),
    ([1024.0, 2.0, 2.0], 5.0, 2.0, 0.5, 3, [2048.0, 0.0, 3.0]),                 # growth at `interval` good steps in a row
    ([1024.0, 2.0, 7.0], INF, 2.0, 0.5, 3, [512.0, 0.0, 7.0]),                  # back off, tracker reset, nothing counted
    ([1024.0, 2.0, 7.0], NAN, 2.0, 0.5, 3, [512.0, 0.0, 7.0]),
    ([1024.0, 2.0, 7.0], -INF, 2.0, 0.5, 3, [512.0, 0.0, 7.0]),
    ([1024.0, 2.0, 7.0], 1e301, 2.0, 0.5, 3, [2048.0, 0.0, 8.0]),               # finite: a good step, as the step kernels apply it
    ([2.0 ** 24, 2.0, 9.0], 1.0, 2.0, 0.5, 3, [2.0 ** 24, 0.0, 10.0]),          # the cap
    ([2.0 ** 23, 0.0, 9.0], 1.0, 4.0, 0.5, 1, [2.0 ** 24, 0.0, 10.0]),
    ([1.0, 1.0, 4.0], INF, 2.0, 0.5, 3, [1.0, 0.0, 4.0]),                       # the floor
    ([1.5, 1.0, 4.0], NAN, 2.0, 0.5, 3, [1.0, 0.0, 4.0]),
    ([8.0, 0.0, 0.0], 1.0, 2.0, 0.5, 1, [16.0, 0.0, 1.0]),                      # interval = 1: every good step grows
    ([16.0, 0.0, 1.0], 1.0, 2.0, 0.5, 1, [32.0, 0.0, 2.0]),
    ([8.0, 0.0, 0.0], 1.0, 1.0, 1.0, 2, [8.0, 1.0, 1.0]),                       # growth = backoff = 1: the scale never moves
    ([8.0, 1.0, 1.0], INF, 1.0, 1.0, 2, [8.0, 0.0, 1.0]),
    ([1000.0, 0.0, 0.0], INF, 2.0, 0.3, 2, [float(np.float32(1000.0) * np.float32(0.3)), 0.0, 0.0]),   # one f32 product
]
# a ten-step walk, overflowed and good steps mixed: interval 2, growth 2, backoff 0.5
LOSS_SCALE_WALK = [1.0, INF, 1.0, 1.0, NAN, INF, 1.0, 2.0, 3.0, INF]
LOSS_SCALE_WALK_STATES = [[64.0, 1.0, 1.0], [32.0, 0.0, 1.0], [32.0, 1.0, 2.0], [64.0, 0.0, 3.0], [32.0, 0.0, 3.0], [16.0, 0.0, 3.0],
                          [16.0, 1.0, 4.0], [32.0, 0.0, 5.0], [32.0, 1.0, 6.0], [16.0, 0.0, 6.0]]


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def make_inputs(n, seed, first_step):
    """p, m, v, g as f32 arrays.  Magnitudes are spread over decades (|p| from 1e-5 to a few, |g| from 1e-6 to 10), since an
    error in the update hides behind u|p| where |p| ~ 1.  Planted, by i % 11: 2: g == 0; 4: g == 0 with m == v == 0 (denom == eps,
    the update is 0); 6: p == 0; 8: p == 0 and g == 0.  first_step: m = v = 0 everywhere."""
    rng = np.random.default_rng(20250000 + 7919 * int(seed) + int(n) % 100003)

    def spread(lo, hi):
        return rng.standard_normal(n).clip(-3, 3) * 10.0 ** rng.uniform(lo, hi, n)

    p = spread(-5, 0)
    g = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 1, n)
    m = spread(-6, 0)
    v = (10.0 ** rng.uniform(-6, 0, n)) ** 2
    if first_step:
        m[:], v[:] = 0.0, 0.0
    i = np.arange(n) % 11
    g[(i == 2) | (i == 4) | (i == 8)] = 0.0
    m[i == 4] = 0.0
    v[i == 4] = 0.0
    p[(i == 6) | (i == 8)] = 0.0
    return tuple(a.astype(np.float32) for a in (p, m, v, g))


def single_group_cases():
    """(name, n, hyper set, step, clip case, first_step) of the single-group matrix: every hyper set x every step at the x50
    clip, every clip case at the model's own set, each once at m = v = 0 and once with a state; n = 257 (two blocks, the
    planted specials 23 times over)."""
    out = []
    for first in (True, False):
        for h in (HYPER_MODEL, HYPER_WD0, HYPER_B1_0, HYPER_LR0):
            for step in STEPS + (BIG_STEP,):
                out.append((f"h{h}-t{step}-x50-{'first' if first else 'state'}", 257, h, step, CLIP_X50, first))
        for clip in CLIP_CASES:
            out.append((f"h0-t2-{clip[0]}-{'first' if first else 'state'}", 257, HYPER_MODEL, 2, clip, first))
    return out


# ---------------------------------------------------------------------------------------------
# run tables of uclstm_adamw_step_groups
# ---------------------------------------------------------------------------------------------
def _table(bounds, groups):
    """Runs from the ascending boundaries [0, b1, ..., n] and one group per run."""
    assert len(bounds) == len(groups) + 1
    return np.array([(bounds[i], bounds[i + 1], groups[i]) for i in range(len(groups))], dtype=np.int64)


def _short_runs(rng, start, total, n_groups):
    """Boundaries of runs of lengths 1..7 (mean 3.2) from `start` until at least `total` elements are covered."""
    lens = rng.choice([1, 1, 1, 2, 2, 3, 4, 5, 6, 7], size=total)            # more than enough
    ends = start + np.cumsum(lens)
    ends = ends[:int(np.searchsorted(ends, start + total)) + 1]
    return [int(e) for e in ends]


def run_table_cases():
    """(name, n, runs i64 [n_runs][3], n_groups), each asserting here that it reaches what it is meant for."""
    rng = np.random.default_rng(4097)
    cases = []
    for n in (1, 1023, 1024, 1025):
        cases.append((f"one-run-n{n}", n, _table([0, n], [0]), 1))
    n = 2 * CHUNK + 37
    for b in (1023, 1024, 1025, 256, 768):                                    # 256, 768: between a lane's own elements
        cases.append((f"two-runs-b{b}", n, _table([0, b, n], [0, 1]), 3))
    cases.append(("single-at-0", n, _table([0, 1, n], [1, 0]), 3))
    cases.append(("single-at-last", n, _table([0, n - 1, n], [0, 2]), 3))
    cases.append(("single-at-1023", n, _table([0, 1023, 1024, n], [0, 1, 2]), 3))
    cases.append(("single-at-1024", n, _table([0, 1024, 1025, n], [2, 1, 0]), 3))     # n_runs = 3, block 1's chunk begins at a run's begin
    assert cases[5][2][1][0] == CHUNK and cases[-1][2][1][0] == CHUNK
    # at least 300 runs of lengths 1..7 inside chunk 0, groups interleaved: a lane's four elements lie many rows apart
    ends = _short_runs(rng, 0, CHUNK, 3)
    n = 2 * CHUNK + 100
    b = [0] + ends + [n]
    t = _table(b, [k % 3 for k in range(len(b) - 1)])
    assert int(((t[:, 1] <= CHUNK)).sum()) >= 300 and int((t[:, 1] - t[:, 0])[:-1].max()) <= 7
    cases.append(("short-runs-in-one-chunk", n, t, 3))
    # a run over three chunks, then a boundary inside the next chunk
    n = 5 * CHUNK
    t = _table([0, 3 * CHUNK + 300, 4 * CHUNK + 50, n], [0, 1, 2])
    assert t[0][1] - t[0][0] > 3 * CHUNK and t[0][1] % CHUNK != 0
    cases.append(("run-over-three-chunks", n, t, 3))
    # a boundary inside the buffer's partial last chunk
    n = 3 * CHUNK + 700
    t = _table([0, 3 * CHUNK + 350, n], [1, 0])
    assert n % CHUNK != 0 and n - n % CHUNK < t[1][0] < n
    cases.append(("boundary-in-partial-chunk", n, t, 3))
    # the second trip of the grid-stride loop: block 0 goes from chunk 0 (run 0) to the chunk at 2 097 152 over several thousand
    # rows; a boundary inside that chunk; the partial last chunk is block 1's second trip and has a boundary too
    n = GROUPS_SWEEP + CHUNK + 5
    ends = _short_runs(rng, 100 * CHUNK + 17, 16000, 3)
    b = [0, 100 * CHUNK + 17] + ends + [GROUPS_SWEEP + 512, GROUPS_SWEEP + CHUNK + 2, n]
    t = _table(b, [k % 3 for k in range(len(b) - 1)])
    assert n > GROUPS_SWEEP and n % CHUNK != 0 and n - n % CHUNK >= GROUPS_SWEEP
    assert int(((t[:, 0] >= CHUNK) & (t[:, 1] <= GROUPS_SWEEP)).sum()) >= 4000
    assert any(GROUPS_SWEEP < int(x) < GROUPS_SWEEP + CHUNK for x in t[:, 0]) and any(n - n % CHUNK < int(x) < n for x in t[:, 0])
    cases.append(("second-trip", n, t, 3))
    # n_runs = 4097 (a 13-step binary search), 257 and 1024 groups (the LDS fill loop's 2nd .. 4th trips); runs of 4 elements, so
    # every block but the first begins its first chunk exactly at a run's begin
    for ng in (257, MAX_GROUPS):
        nr = 4097
        b = [4 * k for k in range(nr + 1)]
        t = _table(b, [k % ng for k in range(nr)])
        assert ng > LDS_FILL and len(set(t[:, 2].tolist())) == ng and any(int(x) % CHUNK == 0 and x > 0 for x in t[:, 0])
        cases.append((f"runs4097-groups{ng}", 4 * nr, t, ng))
    assert {c[3] for c in cases} == {1, 3, 257, 1024} and {1, 2, 3, 4097} <= {len(c[2]) for c in cases}
    return cases
