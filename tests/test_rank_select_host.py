"""CPU-only tests of the dataset statistics: numpy's float32 percentile pinned to the rank rule the device path uses, the
monotone-transform shortcut behind trans_min / trans_max, the argument contract of the entry points that needs no launch, and
the C ABI entries."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import engine as E

import rank_select_cases as R

F32 = np.float32


def _arrays():
    """A few hundred small arrays: interleaved signs, zero-heavy, long runs, constant, denormal, +-x pairs, of lengths 1 .. 3000."""
    rng = np.random.default_rng(7)
    out = []
    for i in range(240):
        n = int(rng.integers(1, 3001)) if i >= 8 else i + 1
        name = ["mixed", "zero_heavy", "run", "equal", "denormal", "pairs"][i % 6]
        out.append(R.value_set(name, n, seed=i))
    return out


def test_the_f32_rank_rule_is_numpy_percentile_bit_for_bit():
    bad = []
    for v in _arrays():
        for absolute in (False, True):
            a = np.abs(v) if absolute else v
            s = np.sort(a)
            for q in R.QS:
                want = np.percentile(a, q)
                assert want.dtype == F32
                lo, hi, g = R.ranks_for(s.size, q)
                got = R.lerp(s[lo], s[hi], g)
                # the package's own helpers are the same rule
                plo, phi, pg = E.percentile_ranks(s.size, q)
                got2 = E.percentile_lerp(s[plo], s[phi], pg)
                if F32(got).tobytes() != F32(want).tobytes() or F32(got2).tobytes() != F32(want).tobytes():
                    bad.append((s.size, q, absolute, float(got), float(got2), float(want)))
    assert not bad, bad[:5]


def test_the_rank_rule_above_2_pow_24_elements_is_numpys_rounded_rank():
    n = (1 << 24) + 12345
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(n) * 3).astype(F32)
    v[rng.random(n) < 0.6] = 0.0
    s = np.sort(v)
    rounded = 0
    for q in R.QS:
        want = np.percentile(v, q)
        lo, hi, g = R.ranks_for(n, q)
        assert (lo, hi) == E.percentile_ranks(n, q)[:2] and 0 <= lo <= hi <= n - 1
        assert F32(R.lerp(s[lo], s[hi], g)).tobytes() == F32(want).tobytes(), (q, lo, hi)
        elo, ehi, eg = E.percentile_ranks(n, q, exact=True)
        assert isinstance(eg, np.float64) and elo == min(int(np.floor((n - 1) * (q / 100.0))), n - 1)
        rounded += (elo, ehi) != (lo, hi)
    assert rounded > 0          # the f32 rank really is another element somewhere: parity reproduces it, exact=True does not


@pytest.mark.parametrize("transform", ["asinh", "signed_log"])
def test_percentile_of_the_transformed_array_is_the_transform_of_two_order_statistics(transform):
    def fwd(a, scale):
        if transform == "asinh":
            return np.arcsinh(a / scale)
        return np.sign(a) * np.log1p(np.abs(a) / scale)
    for i, v in enumerate(_arrays()[::3]):
        scale = float(np.percentile(np.abs(v), 99)) or 1.0
        yt = fwd(v, scale)
        assert yt.dtype == F32
        assert np.all(np.diff(fwd(np.sort(v), scale)) >= 0)                 # monotone non-decreasing in f32
        s = np.sort(v)
        for q in R.QS:
            lo, hi, g = R.ranks_for(s.size, q)
            a, b = fwd(np.array([s[lo], s[hi]], dtype=F32), scale)          # numpy on a 2-element array: the same bits
            assert F32(R.lerp(a, b, g)).tobytes() == F32(np.percentile(yt, q)).tobytes(), (i, q)


def test_key_model_orders_like_numpy_and_round_trips():
    v = np.concatenate([R.value_set(k, 500, seed=1) for k in ("mixed", "denormal", "inf", "zeros", "pairs")])
    for kind, a in (("signed", v), ("abs", np.abs(v))):
        got = R.value_of(np.sort(R.keys_of(v, kind)))
        want = np.sort(a)
        assert R.same_bits(got, want.view(np.uint32))
    assert R.keys_of(R.value_set("nan", 200), "signed").size == int((~np.isnan(R.value_set("nan", 200))).sum())


def test_abi_entries_exist_and_the_version_is_unchanged():
    spec = importlib.util.spec_from_file_location("uclstm_build_for_test", os.path.join(os.path.dirname(L.__file__), "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "dataset_stats.hip" in build.SOURCES and "dataset_stats.hip" not in build.F16_SOURCES
    for sym in ("uclstm_select_workspace_bytes", "uclstm_select_begin", "uclstm_select_accumulate", "uclstm_select_narrow",
                "uclstm_select_finish", "uclstm_dataset_extremes_begin", "uclstm_dataset_extremes"):
        assert sym in L._PROTOS and sym in L.header_symbols() and hasattr(L.lib, sym), sym
        assert sym not in L._ALL_F16_TWINS and not hasattr(C.CDLL(L.LIB_PATH), sym + "_f16")
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16            # additive change
    assert L.lib.uclstm_select_workspace_bytes() == 8 * (L.SELECT_WS_HIST + L.SELECT_MAX_SLOTS * L.SELECT_BINS)
    with open(L.HEADER_PATH) as f:
        header = f.read()
    for name, value in (("SELECT_MAX_SLOTS", L.SELECT_MAX_SLOTS), ("SELECT_BINS", L.SELECT_BINS), ("SELECT_ABS", L.SELECT_ABS),
                        ("SELECT_WS_PREFIX", L.SELECT_WS_PREFIX), ("SELECT_WS_RANK", L.SELECT_WS_RANK),
                        ("SELECT_WS_LEADER", L.SELECT_WS_LEADER), ("SELECT_WS_HIST", L.SELECT_WS_HIST),
                        ("EXTREMES_NONZERO", L.EXTREMES_NONZERO), ("EXTREMES_COUNT", L.EXTREMES_COUNT), ("EXTREMES_WORDS", L.EXTREMES_WORDS)):
        assert f"#define UCLSTM_{name} {value}\n" in header, name
    for name in ("DeviceNPZDataset", "device_order_statistics", "device_percentile", "device_extremes"):
        assert name in U.__all__ and hasattr(U, name)


def test_bad_arguments_are_refused_before_any_launch():
    """Every refusal happens on the host side of the entry point, so it can be asserted without a device: the pointers below are
    never dereferenced."""
    st = L.SelectState()
    ws, v = C.c_void_p(0x1000), C.c_void_p(0x2000)
    ranks, kinds = (C.c_int64 * 8)(*range(8)), (C.c_int32 * 8)(*([0, 1] * 4))
    bad = L.lib.uclstm_select_begin
    assert bad(None, ws, ranks, kinds, 2, None) == -1
    assert bad(C.byref(st), None, ranks, kinds, 2, None) == -1
    assert bad(C.byref(st), C.c_void_p(0x1004), ranks, kinds, 2, None) == -1          # misaligned workspace
    assert bad(C.byref(st), ws, None, kinds, 2, None) == -1
    assert bad(C.byref(st), ws, ranks, None, 2, None) == -1
    for n_slots in (0, -1, 9):
        assert bad(C.byref(st), ws, ranks, kinds, n_slots, None) == -1
    assert bad(C.byref(st), ws, ranks, (C.c_int32 * 2)(0, 2), 2, None) == -1           # unknown kind
    # a state that begin has not set up
    assert L.lib.uclstm_select_accumulate(C.byref(st), 0, v, 4, None) == -1
    assert L.lib.uclstm_select_narrow(C.byref(st), 0, None) == -1
    assert L.lib.uclstm_select_finish(C.byref(st), v, v, None) == -1
    # a state as begin leaves it (written by hand: begin itself launches)
    st.workspace, st.n_slots, st.abs_mask, st.phase, st.magic = 0x1000, 2, 0, 0, 0x53454c31
    acc = L.lib.uclstm_select_accumulate
    assert acc(None, 0, v, 4, None) == -1
    assert acc(C.byref(st), 0, None, 4, None) == -1
    assert acc(C.byref(st), 0, C.c_void_p(0x2002), 4, None) == -1                      # no f32 pointer
    assert acc(C.byref(st), 0, v, -1, None) == -1
    assert acc(C.byref(st), 0, v, 1 << 31, None) == -1
    for p in (-1, 1, 2, 3):                                                            # pass out of order
        assert acc(C.byref(st), p, v, 4, None) == -1
        assert L.lib.uclstm_select_narrow(C.byref(st), p, None) == -1
    assert L.lib.uclstm_select_finish(C.byref(st), v, v, None) == -1                   # finish before narrow(2)
    st.phase = 3
    assert L.lib.uclstm_select_finish(C.byref(st), None, v, None) == -1
    assert L.lib.uclstm_select_finish(C.byref(st), v, None, None) == -1
    assert acc(C.byref(st), 2, v, 4, None) == -1
    assert st.phase == 3 and st.magic == 0x53454c31                                    # refusals change nothing
    ext = L.lib.uclstm_dataset_extremes
    assert L.lib.uclstm_dataset_extremes_begin(None, None) == -1
    assert ext(None, 4, v, None) == -1 and ext(v, 4, None, None) == -1 and ext(v, -1, v, None) == -1 and ext(v, 1 << 31, v, None) == -1
    assert ext(v, 4, C.c_void_p(0x2004), None) == -1


def test_python_argument_checks_need_no_device():
    with pytest.raises(ValueError):
        E.device_percentile([], 101.0)
    assert E.percentile_ranks(1, 50)[:2] == (0, 0) and E.percentile_ranks(10, 100)[:2] == (9, 9) and E.percentile_ranks(10, 0)[:2] == (0, 1)
