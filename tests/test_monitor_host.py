"""StepMonitor, host side (no GPU): the two entry points in the header, the ctypes table and the library, their argument contract
before any launch, the block tables of build_stat_blocks / check_stat_blocks, attach_monitor's validation, StepMonitor.reduce on
hand-made rings, and the f64 restatement of tests/monitor_cases.py against closed forms."""
import ctypes as C
import math
import re
import types

import numpy as np
import pytest

import monitor_cases as M
import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import build as B
from unet_convlstm_amd.optim import FusedAdamW, StepMonitor, build_stat_blocks, check_monitor, check_stat_blocks

ARITY = {"uclstm_param_stats_chunk": 0, "uclstm_param_stats": 16}
CHUNK = M.chunk()


def test_header_ctypes_table_and_library_agree_and_the_abi_version_stays():
    hdr = open(L.HEADER_PATH).read()
    assert int(re.search(r"#define UCLSTM_ABI_VERSION (\d+)", hdr).group(1)) == 16 == L.ABI_VERSION == L.lib.uclstm_abi_version()
    raw = C.CDLL(L.LIB_PATH)
    for sym, arity in ARITY.items():
        assert sym in L._PROTOS and sym in L.header_symbols() and hasattr(raw, sym), sym
        m = re.search(r"int(?:32|64)_t %s\(([^)]*)\);" % sym, hdr)
        assert m is not None, sym
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in params.split(",") if a.strip() not in ("", "void")]) == len(L._PROTOS[sym]) == arity, sym
        assert sym not in L._ALL_F16_TWINS and sym + "_f16" not in L.header_symbols() and not hasattr(raw, sym + "_f16")
    assert L._RESTYPES["uclstm_param_stats_chunk"] is C.c_int64
    assert "param_stats.hip" in B.SOURCES and "param_stats.hip" not in B.F16_SOURCES
    assert U.StepMonitor is StepMonitor and "StepMonitor" in U.__all__
    # the row and the state layout are written down where the entry points are declared
    assert "{every, steps_seen, records_done" in hdr and "{tensor, start, count}" in hdr and "{first_block, n_blocks_of_tensor}" in hdr


def test_chunk_is_positive_and_a_multiple_of_the_block():
    assert CHUNK > 0 and CHUNK % 256 == 0
    assert int(L.lib.uclstm_param_stats_chunk()) == CHUNK                 # a constant: it launches nothing and depends on nothing


def test_entry_point_validates_before_any_launch():
    """Null device pointers throughout: every call returns its code before a launch could dereference anything."""
    stats = L.lib.uclstm_param_stats
    host = (C.c_double * 64)()                       # host memory, 16-byte aligned part of it: never dereferenced
    a = C.addressof(host)
    a += (-a) % 16
    q = C.c_void_p(a)
    ok = [q, q, None, 16, q, 1, q, 1, q, q, q, 4, None, None, q, None]
    for i, bad in ((0, None), (1, None), (4, None), (6, None), (8, None), (9, None), (10, None), (14, None),
                   (3, 0), (3, -5), (5, 0), (5, -1), (7, 0), (7, -1), (11, 0), (11, -3),
                   (0, C.c_void_p(a + 4)), (1, C.c_void_p(a + 8)), (2, C.c_void_p(a + 4)), (8, C.c_void_p(a + 8))):      # misaligned p / g / prev / partials
        args = list(ok)
        args[i] = bad
        assert stats(*args) == -1, (i, bad)
    # with nothing usable at all
    assert stats(None, None, None, 0, None, 0, None, 0, None, None, None, 0, None, None, None, None) == -1
    assert all(v == 0.0 for v in host)


SIZE_CASES = [[n] for n in M.abi_sizes(CHUNK)] + [M.abi_sizes(CHUNK), M.abi_layout(CHUNK), [3 * CHUNK + 5, 1, CHUNK, CHUNK - 1, 1, CHUNK + 1]]


@pytest.mark.parametrize("sizes", SIZE_CASES, ids=lambda s: "+".join(str(n) for n in s))
def test_build_stat_blocks_covers_every_element_once_in_order(sizes):
    blocks, tensors = build_stat_blocks(sizes, CHUNK)
    assert blocks.dtype == tensors.dtype == np.int64 and blocks.shape[1] == 3 and tensors.shape == (len(sizes), 2)
    n = sum(sizes)
    cover = np.zeros(n, dtype=np.int64)
    owner = np.repeat(np.arange(len(sizes)), sizes)
    for t, start, count in blocks.tolist():
        assert 1 <= count <= CHUNK
        cover[start:start + count] += 1
        assert np.all(owner[start:start + count] == t), "a block straddles two tensors"
    assert np.all(cover == 1)
    assert blocks[:, 1].tolist() == sorted(blocks[:, 1].tolist()) and blocks[:, 0].tolist() == sorted(blocks[:, 0].tolist())
    assert blocks.shape[0] == sum((s + CHUNK - 1) // CHUNK for s in sizes)
    for t, (first, nb) in enumerate(tensors.tolist()):
        assert nb == (sizes[t] + CHUNK - 1) // CHUNK and np.all(blocks[first:first + nb, 0] == t)
        assert blocks[first, 1] == sum(sizes[:t]) and blocks[first:first + nb, 2].sum() == sizes[t]
    check_stat_blocks(blocks, tensors, n, CHUNK)                            # and the checker accepts what the builder makes


def test_build_stat_blocks_refuses_what_cannot_occur():
    for sizes in ([], [4, 0, 2], [3, -1]):
        with pytest.raises(ValueError):
            build_stat_blocks(sizes, CHUNK)
    with pytest.raises(ValueError):
        build_stat_blocks([4], 0)


def test_check_stat_blocks_refuses_each_kind_of_bad_table():
    sizes = [5, CHUNK + 1, 1]
    n = sum(sizes)
    blocks, tensors = build_stat_blocks(sizes, CHUNK)
    check_stat_blocks(blocks, tensors, n, CHUNK)

    def broken(edit):
        b, t = blocks.copy(), tensors.copy()
        out = edit(b, t)
        return out if out is not None else (b, t)

    cases = {
        "a block longer than the chunk": lambda b, t: (np.array([[0, 0, CHUNK + 6], [1, CHUNK + 6, 1]], dtype=np.int64), np.array([[0, 1], [1, 1]], dtype=np.int64)),
        "an empty block": lambda b, t: b.__setitem__((0, 2), 0),
        "a gap": lambda b, t: b.__setitem__((1, 1), 6),
        "an overlap": lambda b, t: b.__setitem__((1, 1), 4),
        "blocks out of order": lambda b, t: (b[[0, 2, 1, 3]], t),
        "a skipped tensor": lambda b, t: b.__setitem__((3, 0), 3),
        "a tensor index that goes back": lambda b, t: b.__setitem__((2, 0), 0),
        "a short cover": lambda b, t: (b[:-1], t[:-1]),
        "a tensor row too many": lambda b, t: (b, np.concatenate([t, [[4, 1]]])),
        "a tensor row that starts late": lambda b, t: t.__setitem__((1, 0), 2),
        "a tensor row one block short": lambda b, t: t.__setitem__((1, 1), 1),
        "a tensor row one block long": lambda b, t: t.__setitem__((0, 1), 2),
        "a tensor row without blocks": lambda b, t: t.__setitem__((2, 1), 0),
        "a table of another type": lambda b, t: (b.astype(np.int32), t),
        "a table of another shape": lambda b, t: (b[:, :2], t),
        "an empty table": lambda b, t: (b[:0], t),
    }
    for what, edit in cases.items():
        b, t = broken(edit)
        with pytest.raises(ValueError, match="stat blocks"):
            check_stat_blocks(b, t, n, CHUNK)
            pytest.fail(f"accepted: {what}")
    with pytest.raises(ValueError, match="stat blocks"):
        check_stat_blocks(blocks, tensors, n + 1, CHUNK)                     # the buffer is longer than the cover
    with pytest.raises(ValueError, match="stat blocks"):
        check_stat_blocks(blocks, tensors, n, CHUNK - 1)                     # a smaller chunk than the table was built for


def test_attach_monitor_validates_like_a_spec():
    assert check_monitor(1, 128, True) == (1, 128, True) and check_monitor(7, 65536, False) == (7, 65536, False)
    assert check_monitor(np.int64(3), np.int32(2), True) == (3, 2, True)
    for bad in (0, -2, 1.0, 2.5, "1", None, True, 1 << 24):
        with pytest.raises(ValueError, match="every"):
            check_monitor(bad, 128, True)
    for bad in (0, -1, 65537, 8.0, "8", None, False):
        with pytest.raises(ValueError, match="history"):
            check_monitor(1, bad, True)
    for bad in (0, 1, None, "yes", np.bool_(True)):
        with pytest.raises(ValueError, match="updates"):
            check_monitor(1, 128, bad)
    # the method validates before it touches the optimiser, and refuses a second monitor
    with pytest.raises(ValueError, match="history"):
        FusedAdamW.attach_monitor(types.SimpleNamespace(monitor=None), history=0)
    with pytest.raises(RuntimeError, match="attached already"):
        FusedAdamW.attach_monitor(types.SimpleNamespace(monitor=object()))


# ---------------------------------------------------------------------------------------------
# StepMonitor.reduce on hand-made rings
# ---------------------------------------------------------------------------------------------
def _hand_ring(history, n, records, scales=None, skipped=()):
    """A ring written the way the device writes it: record r (1-based step 10 * r) into slot (r - 1) % history; column c of
    tensor t holds (r * 100 + t * 10 + c) squared where it is a sum, plainly otherwise."""
    ring, meta = np.zeros((history, n, 8)), np.zeros((history, 4))
    for r in range(1, records + 1):
        slot = (r - 1) % history
        for t in range(n):
            for c in range(8):
                v = float(r * 100 + t * 10 + c)
                ring[slot, t, c] = v * v if c in M.SUM_COLS else v
        scale = 1.0 if scales is None else scales[r - 1]
        meta[slot] = [10 * r, scale, float("inf") if r in skipped else (r * 3.0) ** 2, 1.0 if r in skipped else 0.0]
    return ring, meta


@pytest.mark.parametrize("history,records", [(4, 3), (4, 4), (4, 11), (1, 5), (3, 0)],
                         ids=["fewer-than-history", "exactly-history", "wrapped-twice", "history-1", "no-record"])
def test_reduce_unwinds_the_ring_in_chronological_order(history, records):
    n = 3
    ring, meta = _hand_ring(history, n, records)
    numel = np.array([4, 10, 1000])
    r = StepMonitor.reduce(ring, meta, records, history, True, ["a", "b", "c"], numel, [0, 1, 0])
    kept = list(range(max(1, records - history + 1), records + 1))
    assert r["step"].tolist() == [10 * k for k in kept] and r["step"].dtype == np.int64
    assert r["names"] == ["a", "b", "c"] and r["numel"].tolist() == numel.tolist() and r["group"].tolist() == [0, 1, 0]
    assert r["skipped"].dtype == np.bool_ and not r["skipped"].any() and r["scale"].tolist() == [1.0] * len(kept)
    for key in StepMonitor.PER_TENSOR:
        assert r[key].shape == (len(kept), n), key
    for i, k in enumerate(kept):
        assert r["global_grad_norm"][i] == 3.0 * k
        for t in range(n):
            base = k * 100 + t * 10
            assert r["grad_norm"][i, t] == base and r["grad_max"][i, t] == base + 1 and r["grad_nonfinite"][i, t] == base + 2
            assert r["grad_zero_frac"][i, t] == (base + 3) / numel[t]
            assert r["weight_norm"][i, t] == base + 4 and r["weight_max"][i, t] == base + 5 and r["weight_nonfinite"][i, t] == base + 6
            assert r["update_norm"][i, t] == base + 7 and r["update_ratio"][i, t] == (base + 7) / (base + 4)
    assert r["grad_nonfinite"].dtype == np.int64 and r["weight_nonfinite"].dtype == np.int64


def test_reduce_unscales_gradients_and_flags_skipped_records():
    scales = [1024.0, 1024.0, 512.0, 512.0, 0.5]
    ring, meta = _hand_ring(4, 2, 5, scales=scales, skipped={3})
    r = StepMonitor.reduce(ring, meta, 5, 4, True)
    assert r["step"].tolist() == [20, 30, 40, 50] and r["scale"].tolist() == scales[1:] and r["skipped"].tolist() == [False, True, False, False]
    assert r["names"] == ["param0", "param1"]
    for i, k in enumerate((2, 3, 4, 5)):
        s = scales[k - 1]
        assert r["global_grad_norm"][i] == (math.inf if k == 3 else 3.0 * k / s)
        for t in range(2):
            base = k * 100 + t * 10
            assert r["grad_norm"][i, t] == base / s and r["grad_max"][i, t] == (base + 1) / s
            assert r["weight_norm"][i, t] == base + 4 and r["update_norm"][i, t] == base + 7          # weights are never scaled
    # no global norm in the plain branch: NaN, not an error
    meta[:, 2] = np.nan
    assert np.isnan(StepMonitor.reduce(ring, meta, 5, 4, True)["global_grad_norm"]).all()


def test_reduce_without_updates_reads_nan_and_a_zero_weight_does_not_divide_by_zero():
    ring, meta = _hand_ring(2, 2, 2)
    r = StepMonitor.reduce(ring, meta, 2, 2, False)
    assert np.isnan(r["update_norm"]).all() and np.isnan(r["update_ratio"]).all()
    assert np.isfinite(r["grad_norm"]).all() and np.isfinite(r["weight_norm"]).all()
    ring[:, 0, 4] = 0.0                              # an all-zero tensor that moved: the formula overflows to inf; one that did not: 0
    ring[:, 1, 4], ring[:, 1, 7] = 0.0, 0.0
    r = StepMonitor.reduce(ring, meta, 2, 2, True)
    assert not np.isnan(r["update_ratio"]).any() and (r["update_ratio"][:, 0] > 1e300).all() and (r["update_ratio"][:, 1] == 0.0).all()


# ---------------------------------------------------------------------------------------------
# the restatement against closed forms
# ---------------------------------------------------------------------------------------------
def test_restatement_constant_tensors():
    n = 1000
    g, p = np.full(n, 0.5, dtype=np.float32), np.full(n, -3.0, dtype=np.float32)
    prev = np.full(n, -2.75, dtype=np.float32)
    assert M.tensor_ref(g, p, prev).tolist() == [0.25 * n, 0.5, 0, 0, 9.0 * n, 3.0, 0, 0.0625 * n]
    assert M.tensor_ref(g, p).tolist() == [0.25 * n, 0.5, 0, 0, 9.0 * n, 3.0, 0, 0.0]
    assert M.tensor_ref(g, p, p).tolist()[7] == 0.0                                    # prev == p: no update, exactly
    assert M.tensor_ref(np.zeros(n, dtype=np.float32), p, p).tolist()[:4] == [0.0, 0.0, 0, n]


def test_restatement_planted_values():
    g = np.array([1.0, np.inf, -2.0, np.nan, -0.0, 0.0, -np.inf, 2.0 ** -140], dtype=np.float32)
    p = np.array([np.nan, 1.0, 3.0, -4.0, np.inf, 0.5, 0.25, -0.0], dtype=np.float32)
    q = np.array([1.0, np.inf, 1.0, -4.0, 0.0, np.nan, 0.75, 0.0], dtype=np.float32)
    row = M.tensor_ref(g, p, q)
    assert row[0] == 1.0 + 4.0 + 2.0 ** -280 and row[1] == 2.0 and row[2] == 3 and row[3] == 2
    assert row[4] == 1.0 + 9.0 + 16.0 + 0.25 + 0.0625 and row[5] == 4.0 and row[6] == 2
    assert row[7] == 4.0 + 0.0 + 0.25 + 0.0           # pairs (3, 1), (-4, -4), (0.25, 0.75), (-0, 0): the others have a non-finite side
    allnan = np.full(7, np.nan, dtype=np.float32)
    assert M.tensor_ref(allnan, allnan, allnan).tolist() == [0.0, 0.0, 7, 0, 0.0, 0.0, 7, 0.0]


def test_restatement_of_a_whole_call_walks_the_ring_and_the_counters():
    sizes = [3, 5]
    rng = np.random.default_rng(0)
    p = rng.integers(-8, 8, 8).astype(np.float32)              # eighths stay exact in f32
    g = rng.standard_normal(8).astype(np.float32)
    prev0 = p.copy()
    ring, meta, state, prev = np.zeros((2, 2, 8)), np.zeros((2, 4)), M.make_state(3), prev0
    seen_prev = []
    for call in range(1, 9):
        p = (p + np.float32(0.125)).astype(np.float32)
        ring, meta, state, prev, rec = M.call_ref(p, g, prev, sizes, ring, meta, state, 2, sumsq=float(call), scale=2.0)
        assert rec == (call % 3 == 0) and state[M.I_SEEN] == call and state[M.I_DONE] == call // 3
        seen_prev.append(prev.copy())
    assert np.array_equal(seen_prev[0], prev0) and np.array_equal(seen_prev[1], prev0) and not np.array_equal(seen_prev[2], prev0)
    assert meta[:, 0].tolist() == [3.0, 6.0] and meta[:, 1].tolist() == [2.0, 2.0] and meta[:, 2].tolist() == [3.0, 6.0] and not meta[:, 3].any()
    assert ring[1, 0, 7] == 3 * (3 * 0.125) ** 2 and ring[1, 1, 7] == 5 * (3 * 0.125) ** 2          # the change over calls 4..6
    r = StepMonitor.reduce(ring, meta, int(state[M.I_DONE]), 2)
    assert r["step"].tolist() == [3, 6]
    # an overflowed sum of squares is flagged, a missing one is NaN and not flagged; without prev nothing is rewritten
    _, meta2, _, none, _ = M.call_ref(p, g, None, sizes, ring, meta, M.make_state(1), 2, sumsq=float("nan"))
    assert none is None and np.isnan(meta2[0, 2]) and meta2[0, 3] == 1.0 and meta2[0, 1] == 1.0
    _, meta3, _, _, _ = M.call_ref(p, g, None, sizes, ring, meta, M.make_state(1), 2)
    assert np.isnan(meta3[0, 2]) and meta3[0, 3] == 0.0
    for ss, skipped in ((s, k) for s, _, k in M.META_CASES if s is not None):
        assert M.overflowed(ss) == skipped


def test_planted_values_reach_block_edges_and_every_offset():
    sizes = M.abi_layout(CHUNK)
    assert set(M.abi_sizes(CHUNK)) <= set(sizes)
    assert {int(o) % 4 for o in M.offsets_of(sizes)} == {0, 1, 2, 3}
    nan_t = len(sizes) - 1
    g, p, prev = M.planted(sizes, CHUNK, seed=1, nan_tensor=nan_t)
    blocks, _ = build_stat_blocks(sizes, CHUNK)
    firsts, lasts = blocks[:, 1], blocks[:, 1] + blocks[:, 2] - 1
    for arr in (g, p, prev):
        for edge in (firsts, lasts):
            v = arr[edge]
            assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
            assert (v == 0).any() and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
            assert ((np.abs(v) < np.finfo(np.float32).tiny) & (v != 0)).any()
    o = int(M.offsets_of(sizes)[nan_t])
    assert np.isnan(g[o:]).all() and np.isnan(p[o:]).all()
    assert np.isfinite(g).mean() > 0.99                                                # and almost everything is an ordinary number
