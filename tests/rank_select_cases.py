"""Shared cases of the rank-select tests and a numpy model of what the kernels compute: the order-preserving u32 key of an f32
(csrc/dataset_stats.hip), numpy's own rank rule for float32 percentiles, and its interpolation."""
import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------
# the key model
# ---------------------------------------------------------------------------------------------
def is_nan_bits(bits):
    return (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def keys_of(v, kind="signed"):
    """u32 keys of the NON-NaN elements of the f32 array ``v``: -0.0 is +0.0, negatives have all bits inverted, the others the
    sign bit set; ``kind='abs'`` clears the sign first."""
    bits = np.ascontiguousarray(v, dtype=F32).reshape(-1).view(np.uint32)
    bits = bits[~is_nan_bits(bits)].copy()
    if kind == "abs":
        return (bits & np.uint32(0x7fffffff)) | np.uint32(0x80000000)
    bits[bits == np.uint32(0x80000000)] = 0
    neg = (bits & np.uint32(0x80000000)) != 0
    return np.where(neg, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def value_of(keys):
    """The f32 behind a key (a zero comes back as +0.0)."""
    k = np.asarray(keys, dtype=np.uint32).reshape(-1)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def order_statistics(v, ranks, kinds):
    """What the select must return, as u32 BIT PATTERNS: np.sort of the key image, indexed, decoded."""
    cache = {}
    out = []
    for r, k in zip(ranks, kinds):
        if k not in cache:
            cache[k] = np.sort(keys_of(v, k))
        out.append(value_of(cache[k][r:r + 1])[0])
    return np.array(out, dtype=F32).view(np.uint32)


def same_bits(got, want_bits):
    """Bit-identical, a zero of either sign counting as equal."""
    g = np.ascontiguousarray(got, dtype=F32).view(np.uint32).copy()
    w = np.asarray(want_bits, dtype=np.uint32).copy()
    g[g == np.uint32(0x80000000)] = 0
    w[w == np.uint32(0x80000000)] = 0
    return bool(np.array_equal(g, w))


# ---------------------------------------------------------------------------------------------
# numpy's percentile, from two order statistics
# ---------------------------------------------------------------------------------------------
def ranks_for(n, q):
    """(lo, hi, g) of np.percentile(a, q) for a float32 a of n elements, all arithmetic in float32:
    vi = f32(n-1) * (f32(q) / f32(100)); lo = floor(vi), hi = min(lo+1, n-1), g = vi - lo; at or past the last element both
    ranks are n-1 (numpy indexes it as -1 and forms g from that index; it multiplies a zero difference)."""
    vi = F32(n - 1) * (F32(q) / F32(100))
    if vi >= F32(n - 1):
        return n - 1, n - 1, F32(np.float64(vi) + 1.0)
    lo = int(np.floor(vi))
    return lo, min(lo + 1, n - 1), F32(np.float64(vi) - lo)


def lerp(a, b, g):
    a, b, g = F32(a), F32(b), F32(g)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return b - d * (F32(1) - g) if g >= 0.5 else a + d * g


def model_percentile(v, q, absolute=False):
    """np.percentile of a NaN-free f32 array through the rule above and a full sort."""
    s = np.sort(np.abs(v.reshape(-1)) if absolute else v.reshape(-1))
    lo, hi, g = ranks_for(s.size, q)
    return lerp(s[lo], s[hi], g)


QS = [0, 0.00001, 12.5, 50, 99, 99.99999, 100]


# ---------------------------------------------------------------------------------------------
# value sets
# ---------------------------------------------------------------------------------------------
def _bits(*words):
    return np.array(words, dtype=np.uint32).view(F32)


def value_set(name, n, seed=0):
    """``n`` f32 values of one of the named kinds (NaN-free unless the name says so)."""
    rng = np.random.default_rng(seed + n)
    if name == "equal":
        return np.full(n, F32(3.25))
    if name == "zeros":                                         # zeros of both signs
        return np.where(rng.random(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    if name == "low_digit":                                     # two values that differ only in the lowest digit (bits 0..9)
        return _bits(0x40490fdb, 0x40490fda)[rng.integers(0, 2, n)]
    if name == "mid_digit":                                     # ... only in the middle digit (bits 10..20)
        return _bits(0x40490fdb, 0x40491fdb)[rng.integers(0, 2, n)]
    if name == "mixed":                                         # negatives and positives interleaved
        v = (rng.standard_normal(n) * 3).astype(F32)
        v[::2] = -np.abs(v[::2])
        v[1::2] = np.abs(v[1::2])
        return v
    if name == "denormal":
        return (rng.integers(-200, 200, n).astype(np.int64) * 7).astype(F32) * F32(1e-45)
    if name == "inf":
        v = (rng.standard_normal(n) * 3).astype(F32)
        v[rng.random(n) < 0.3] = F32(np.inf)
        v[rng.random(n) < 0.3] = F32(-np.inf)
        return v
    if name == "pairs":                                         # x and -x
        h = np.abs(rng.standard_normal((n + 1) // 2) * 3).astype(F32)
        return rng.permutation(np.concatenate([h, -h]))[:n]
    if name == "run":                                           # a long run of duplicates in the middle of the order
        v = (rng.standard_normal(n) * 3).astype(F32)
        v[rng.random(n) < 0.6] = F32(0.5)
        return v
    if name == "zero_heavy":                                    # the targets of this project: 60 % exact zeros
        v = (rng.standard_normal(n) * 3).astype(F32)
        v[rng.random(n) < 0.6] = 0.0
        return v
    if name == "nan":                                           # NaNs of both signs and several payloads
        v = (rng.standard_normal(n) * 3).astype(F32)
        nans = _bits(0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffa5a5a5)
        at = rng.random(n) < 0.25
        at[0] = True
        v[at] = nans[rng.integers(0, nans.size, int(at.sum()))]
        return v
    raise KeyError(name)


VALUE_SETS = ["equal", "zeros", "low_digit", "mid_digit", "mixed", "denormal", "inf", "pairs", "run", "zero_heavy"]
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 4099, (1 << 20) + 3]


def slot_sets(n):
    """name -> (ranks, kinds) for an array of ``n`` non-NaN elements."""
    mid = n // 2
    eight = [0, n - 1, mid, mid, n // 3, (2 * n) // 3, n - 1, 0]
    return {"ends": ([0, n - 1], ["signed", "signed"]),
            "same_rank_twice": ([mid, mid], ["signed", "signed"]),
            "eight_mixed": (eight, ["signed", "abs", "signed", "abs", "abs", "signed", "abs", "signed"]),
            "single": ([mid], ["abs"])}
