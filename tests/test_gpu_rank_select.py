"""GPU tests of the radix select and the extremes kernel at the C ABI (csrc/dataset_stats.hip): every value must be bit-identical
to np.sort of the key image, indexed and decoded (tests/rank_select_cases.py), a zero of either sign counting as equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import rank_select_cases as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import engine as E
    from unet_convlstm_amd import ops

DEV = "cuda"
F32 = np.float32
KIND = {"signed": 0, "abs": 1}


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _begin(ranks, kinds):
    ws = torch.empty(L.lib.uclstm_select_workspace_bytes() // 8, dtype=torch.int64, device=DEV)
    st = L.SelectState()
    rc = L.lib.uclstm_select_begin(C.byref(st), ops._p(ws), (C.c_int64 * len(ranks))(*ranks),
                                   (C.c_int32 * len(ranks))(*[KIND[k] for k in kinds]), len(ranks), ops._stream())
    assert rc == 0
    return st, ws


def _finish(st, n_slots):
    vals = torch.empty(8, dtype=torch.float32, device=DEV)
    info = torch.empty(4, dtype=torch.int64, device=DEV)
    assert L.lib.uclstm_select_finish(C.byref(st), ops._p(vals), ops._p(info), ops._stream()) == 0
    return vals.cpu().numpy()[:n_slots], info.cpu().numpy().view(np.uint64)


def select(pieces, ranks, kinds):
    """The whole call sequence over ``pieces`` = [(device tensor, element offset, n)], as the header states it."""
    st, ws = _begin(ranks, kinds)
    for p in range(3):
        for t, off, n in pieces:
            assert L.lib.uclstm_select_accumulate(C.byref(st), p, _ptr(t, off), n, ops._stream()) == 0
        assert L.lib.uclstm_select_narrow(C.byref(st), p, ops._stream()) == 0
    return _finish(st, len(ranks))


def _on_device(v, offset=0):
    """``v`` on the device behind ``offset`` leading elements: offset 1 takes the base off the 16-byte boundary."""
    t = torch.empty(v.size + offset + 4, dtype=torch.float32, device=DEV)
    assert t.data_ptr() % 16 == 0
    t[offset:offset + v.size] = torch.from_numpy(v)
    return [(t, offset, v.size)]


def _check(v, ranks, kinds, pieces, what):
    got, info = select(pieces, ranks, kinds)
    want = R.order_statistics(v, ranks, kinds)
    assert R.same_bits(got, want), (what, got, want.view(F32))
    assert int(info[0]) == int(np.isnan(v).sum()) and int(info[1]) == v.size and int(info[2]) == 0, (what, info)


@pytest.mark.parametrize("name", R.VALUE_SETS)
def test_select_is_the_sorted_key_image_at_every_length_and_alignment(name):
    for n in R.LENGTHS:
        v = R.value_set(name, n)
        ranks, kinds = R.slot_sets(n)["eight_mixed"]
        for offset in (0, 1) if n != R.LENGTHS[-1] else (1,):      # the largest: many blocks, scalar head and tail, grid-stride loop
            _check(v, ranks, kinds, _on_device(v, offset), (name, n, offset))
    v = R.value_set(name, (1 << 20) + 3, seed=1)[:(1 << 18) + 4]
    _check(v, *R.slot_sets(v.size)["ends"], _on_device(v, 0), (name, "aligned, several blocks"))


@pytest.mark.parametrize("slots", ["ends", "same_rank_twice", "eight_mixed", "single"])
def test_slot_sets(slots):
    for name in ("run", "zero_heavy", "pairs"):
        v = R.value_set(name, 4099, seed=2)
        ranks, kinds = R.slot_sets(v.size)[slots]
        _check(v, ranks, kinds, _on_device(v), (slots, name))
    v = R.value_set("run", 4099, seed=2)                             # a rank inside the long run of duplicates
    s = np.sort(v)
    inside = int(np.flatnonzero(s == F32(0.5))[100])
    _check(v, [inside, inside + 1], ["signed", "signed"], _on_device(v), "inside the run")
    assert R.order_statistics(v, [inside], ["signed"]).view(F32)[0] == F32(0.5)


def test_nans_are_counted_and_left_out():
    for n in (65, 4099):
        v = R.value_set("nan", n)
        m = int((~np.isnan(v)).sum())
        assert 0 < m < n
        ranks, kinds = [0, m - 1, m // 2, m // 2], ["signed", "signed", "abs", "signed"]
        for offset in (0, 1):
            _check(v, ranks, kinds, _on_device(v, offset), ("nan", n, offset))
        t = torch.from_numpy(v).to(DEV)
        assert np.isnan(U.device_percentile(t, 50.0)) and all(np.isnan(x) for x in U.device_percentile(t, [0.0, 99.0], absolute=True))
        clean = torch.from_numpy(v[~np.isnan(v)]).to(DEV)
        assert R.same_bits(U.device_order_statistics(t, ranks, kinds), R.order_statistics(v, ranks, kinds))
        assert U.device_percentile(clean, 12.5) == float(np.percentile(v[~np.isnan(v)], 12.5))


def test_a_rank_out_of_range_is_flagged_at_finish_and_the_other_slots_stand():
    v = R.value_set("nan", 300)
    m = int((~np.isnan(v)).sum())
    ranks, kinds = [m, 3, -1, m - 1, 1 << 40], ["signed", "abs", "signed", "abs", "abs"]
    got, info = select(_on_device(v), ranks, kinds)
    assert int(info[2]) == 0b10101 and int(info[0]) == 300 - m and int(info[1]) == 300
    assert np.isnan(got[[0, 2, 4]]).all()
    assert R.same_bits(got[[1, 3]], R.order_statistics(v, [3, m - 1], ["abs", "abs"]))
    with pytest.raises(IndexError):
        U.device_order_statistics(torch.from_numpy(v).to(DEV), [0, m], ["signed", "signed"])


def test_pieces_give_the_same_result(monkeypatch):
    v = R.value_set("zero_heavy", 10007, seed=5)
    ranks, kinds = R.slot_sets(v.size)["eight_mixed"]
    want = R.order_statistics(v, ranks, kinds)
    t = torch.from_numpy(v).to(DEV)
    one, info1 = select([(t, 0, v.size)], ranks, kinds)
    cuts = [(t, 0, 3331), (t, 3331, 0), (t, 3331, 4446), (t, 7777, v.size - 7777)]          # odd boundaries and an empty piece
    three, info3 = select(cuts, ranks, kinds)
    assert R.same_bits(one, want) and one.tobytes() == three.tobytes() and info1.tobytes() == info3.tobytes()
    whole = U.device_order_statistics(t, ranks, kinds)
    parts = U.device_order_statistics([t[:3331], t[3331:3331], t[3331:7777], t[7777:]], ranks, kinds)
    monkeypatch.setattr(E, "SELECT_MAX_LAUNCH", 1000)
    log = ops.LAUNCH_LOG = []
    try:
        small = U.device_order_statistics(t, ranks, kinds)
    finally:
        ops.LAUNCH_LOG = None
    assert [e[2:] for e in log if e[:2] == ("select", "accumulate")] == [(p, n) for p in range(3) for n in [1000] * 10 + [7]]
    assert whole.tobytes() == parts.tobytes() == small.tobytes() == one.tobytes()
    ext = U.device_extremes(t)
    assert ext == U.device_extremes([t[:3331], t[3331:3331], t[3331:]]) and len(log) == 33
    with pytest.raises(TypeError):
        U.device_order_statistics(iter([t]), ranks, kinds)


def test_counters_past_2_pow_32_in_narrow():
    """The histogram is written from the host side between the calls: 64-bit counts and ranks with no large array."""
    B = 1 << 32
    ranks, kinds = [5 * B + 17, B - 1, 1 << 40], ["signed", "abs", "signed"]
    st, ws = _begin(ranks, kinds)

    def fill(slot, bins):
        for d, c in bins.items():
            ws[L.SELECT_WS_HIST + slot * L.SELECT_BINS + d] = c

    def ctrl():
        w = ws[:L.SELECT_WS_HIST].cpu().numpy().view(np.uint64)
        return ([int(x) for x in w[L.SELECT_WS_PREFIX:L.SELECT_WS_PREFIX + 3]], [int(x) for x in w[L.SELECT_WS_RANK:L.SELECT_WS_RANK + 3]],
                int(w[L.SELECT_WS_FLAGS]), [int(x) for x in w[L.SELECT_WS_LEADER:L.SELECT_WS_LEADER + 3]])
    assert ctrl()[3] == [0, 1, 0]                                    # slot 2 reads slot 0's counters: same kind, nothing decided yet
    fill(0, {100: 3 * B, 1500: 4 * B + 5, 1501: 2 * B})             # 9 * 2^32 + 5 elements
    fill(1, {1024: B - 1, 1025: 1})
    assert L.lib.uclstm_select_narrow(C.byref(st), 0, ops._stream()) == 0
    prefix, rank, flags, leader = ctrl()
    assert prefix[:2] == [1500 << 21, 1025 << 21] and rank[:2] == [2 * B + 17, 0] and flags == 0b100
    assert leader == [0, 1, (1 << 64) - 1]
    assert int(ws[L.SELECT_WS_HIST:].abs().max()) == 0               # cleared for the next pass
    fill(0, {7: B, 9: B + 18, 10: 3 * B - 13})
    fill(1, {0: 1})
    assert L.lib.uclstm_select_narrow(C.byref(st), 1, ops._stream()) == 0
    prefix, rank, flags, _ = ctrl()
    assert prefix[:2] == [1500 << 21 | 9 << 10, 1025 << 21] and rank[:2] == [B + 17, 0] and flags == 0b100
    fill(0, {3: B + 17, 1023: 1})
    fill(1, {1023: 1})
    assert L.lib.uclstm_select_narrow(C.byref(st), 2, ops._stream()) == 0
    prefix, rank, flags, _ = ctrl()
    keys = [1500 << 21 | 9 << 10 | 1023, 1025 << 21 | 1023]
    assert prefix[:2] == keys and rank[:2] == [0, 0] and flags == 0b100
    got, info = _finish(st, 3)
    assert R.same_bits(got[:2], R.value_of(keys).view(np.uint32)) and np.isnan(got[2]) and int(info[2]) == 0b100


def test_bad_arguments_launch_nothing():
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    ws = torch.empty(L.lib.uclstm_select_workspace_bytes() // 8, dtype=torch.int64, device=DEV)
    out = torch.zeros(8, dtype=torch.int64, device=DEV)
    ranks, kinds = (C.c_int64 * 8)(*([0] * 8)), (C.c_int32 * 8)(*([0, 1] * 4))
    st = L.SelectState()
    s = ops._stream()
    begin, acc, narrow, finish = L.lib.uclstm_select_begin, L.lib.uclstm_select_accumulate, L.lib.uclstm_select_narrow, L.lib.uclstm_select_finish
    for args in ((None, ops._p(ws), ranks, kinds, 2), (C.byref(st), None, ranks, kinds, 2), (C.byref(st), ops._p(ws), None, kinds, 2),
                 (C.byref(st), ops._p(ws), ranks, None, 2), (C.byref(st), ops._p(ws), ranks, kinds, 0), (C.byref(st), ops._p(ws), ranks, kinds, 9),
                 (C.byref(st), ops._p(ws), ranks, (C.c_int32 * 2)(0, 7), 2)):
        assert begin(*args, s) == -1
    assert acc(C.byref(st), 0, ops._p(t), 64, s) == -1               # no begin yet
    assert begin(C.byref(st), ops._p(ws), ranks, kinds, 2, s) == 0
    for args in ((0, None, 64), (0, ops._p(t), -1), (0, ops._p(t), 1 << 31), (1, ops._p(t), 64), (2, ops._p(t), 64), (3, ops._p(t), 64)):
        assert acc(C.byref(st), *args, s) == -1
    assert narrow(C.byref(st), 1, s) == -1 and finish(C.byref(st), ops._p(out), ops._p(out), s) == -1
    assert acc(C.byref(st), 0, ops._p(t), 64, s) == 0 and narrow(C.byref(st), 0, s) == 0
    assert acc(C.byref(st), 0, ops._p(t), 64, s) == -1 and narrow(C.byref(st), 0, s) == -1 and narrow(C.byref(st), 2, s) == -1
    assert acc(C.byref(st), 1, ops._p(t), 64, s) == 0 and acc(C.byref(st), 1, ops._p(t), 0, s) == 0 and narrow(C.byref(st), 1, s) == 0
    assert acc(C.byref(st), 2, ops._p(t), 64, s) == 0 and narrow(C.byref(st), 2, s) == 0
    assert finish(C.byref(st), None, ops._p(out), s) == -1 and finish(C.byref(st), ops._p(out), None, s) == -1
    assert finish(C.byref(st), C.c_void_p(out.data_ptr() + 32), ops._p(out), s) == 0
    assert finish(C.byref(st), C.c_void_p(out.data_ptr() + 32), ops._p(out), s) == -1        # the state has ended
    ext = L.lib.uclstm_dataset_extremes
    assert ext(None, 4, ops._p(out), s) == -1 and ext(ops._p(t), 4, None, s) == -1 and ext(ops._p(t), 1 << 31, ops._p(out), s) == -1
    assert ext(ops._p(t), -1, ops._p(out), s) == -1 and L.lib.uclstm_dataset_extremes_begin(None, s) == -1
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[4:].view(F32)[0] == 0.0 and int(host[1]) == 64       # the one complete select ran on 64 zeros


@pytest.mark.parametrize("name", R.VALUE_SETS + ["nan"])
def test_extremes_match_numpy(name):
    for n in (1, 63, 257, 4099, (1 << 18) + 5):
        v = R.value_set(name, n)
        t = torch.empty(n + 5, dtype=torch.float32, device=DEV)
        for offset in (0, 1):
            t[offset:offset + n] = torch.from_numpy(v)
            view = t[offset:offset + n]
            got = U.device_extremes(view)
            pieces = U.device_extremes([view[:n // 3], view[n // 3:n // 3], view[n // 3:]])
            assert got == pieces or (np.isnan(got["min"]) and np.isnan(pieces["min"])), (name, n, offset)
            ok = v[~np.isnan(v)]
            assert got["count"] == n and got["nan_count"] == int(np.isnan(v).sum()) and got["nonzero"] == int(np.count_nonzero(v)), (name, n, got)
            if ok.size:
                assert R.same_bits([got["min"], got["max"]], np.array([ok.min(), ok.max()], dtype=F32).view(np.uint32)), (name, n, got)
            else:
                assert np.isnan(got["min"]) and np.isnan(got["max"])
