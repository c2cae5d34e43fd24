"""Weight EMA, host side (no GPU): the two entry points in the header, the ctypes table and the library, their argument
contracts before any launch, attach_ema's validation, the f64 restatement of tests/ema_cases.py against closed forms, and the
key set of WeightEMA.model_state_dict on a CPU model."""
import ctypes as C
import math
import re
import types

import numpy as np
import pytest
import torch

import ema_cases as E
import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd.optim import FlatParams, FusedAdamW, WeightEMA, check_ema

ARITY = {"uclstm_ema_update": 6, "uclstm_swap_f32": 4}


def test_header_ctypes_table_and_library_agree_and_the_abi_version_stays():
    hdr = open(L.HEADER_PATH).read()
    assert int(re.search(r"#define UCLSTM_ABI_VERSION (\d+)", hdr).group(1)) == 16 == L.ABI_VERSION == L.lib.uclstm_abi_version()
    raw = C.CDLL(L.LIB_PATH)
    for sym, arity in ARITY.items():
        assert sym in L._PROTOS and sym in L.header_symbols() and hasattr(raw, sym), sym
        m = re.search(r"int32_t %s\(([^)]*)\)" % sym, hdr)
        assert m is not None, sym
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(L._PROTOS[sym]) == arity, sym
        assert sym not in L._ALL_F16_TWINS and sym + "_f16" not in L.header_symbols()
    assert U.WeightEMA is WeightEMA and "WeightEMA" in U.__all__


def test_entry_points_validate_before_any_launch():
    buf = (C.c_float * 64)()                       # host memory: never dereferenced, every call returns before a launch
    base = C.addressof(buf)
    p, q = C.c_void_p(base), C.c_void_p(base + 128)
    upd = L.lib.uclstm_ema_update
    ok = [p, q, 16, None, p, None]
    for i, bad in ((0, None), (1, None), (4, None), (2, -1), (2, 0)):
        args = list(ok)
        args[i] = bad
        assert upd(*args) == -1, (i, bad)
    swap = L.lib.uclstm_swap_f32
    for args in ((None, q, 16, None), (p, None, 16, None), (p, q, -1, None), (p, p, 16, None), (p, p, 0, None),
                 (p, C.c_void_p(base + 4), 2, None),                 # b begins inside a
                 (C.c_void_p(base + 60), p, 16, None),               # a begins at b's last element
                 (p, q, 33, None), (q, p, 33, None)):                # 32 elements apart, 33 long: one element shared
        assert swap(*args) == -1, args
    assert swap(p, q, 0, None) == 0                                  # nothing to do: success, no launch
    assert all(v == 0.0 for v in buf)


def test_attach_ema_validates_like_a_spec():
    assert check_ema(0.999, 10.0, 1) == (0.999, 10.0, 1) and check_ema(0.5, 0, 7) == (0.5, 0.0, 7)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), "0.9", None, True, 1.0 - 2.0 ** -30):
        with pytest.raises(ValueError, match="decay"):
            check_ema(bad, 10.0, 1)
    for bad in (-1.0, float("inf"), float("nan"), "3", None, False):
        with pytest.raises(ValueError, match="warmup"):
            check_ema(0.9, bad, 1)
    for bad in (0, -2, 1.0, 2.5, "1", None, True, 1 << 24):
        with pytest.raises(ValueError, match="every"):
            check_ema(0.9, 10.0, bad)
    # the method validates before it touches the optimiser, and refuses a second EMA
    with pytest.raises(ValueError, match="decay"):
        FusedAdamW.attach_ema(types.SimpleNamespace(ema=None), decay=2.0)
    with pytest.raises(RuntimeError, match="attached already"):
        FusedAdamW.attach_ema(types.SimpleNamespace(ema=object()))


def test_restatement_constant_weights_converge_geometrically():
    rng = np.random.default_rng(1)
    e0, p = rng.standard_normal(50), rng.standard_normal(50)
    state = E.make_state(0.9, 0.0, 1)
    d = float(np.float32(0.9))
    e = e0.copy()
    for k in range(1, 41):
        e, state, dk = E.ema_ref(e, p, state)
        assert dk == np.float32(0.9)                                  # warmup = 0: plain decay, every time
        np.testing.assert_allclose(e - p, (e0 - p) * d ** k, rtol=1e-12, atol=0)
    assert state[E.I_SEEN] == 40 and state[E.I_DONE] == 40


def test_restatement_warmup_decay_is_rounded_once():
    state = E.make_state(0.999, 10.0, 1)
    for k in range(1, 40):
        want = np.float32(min(float(np.float32(0.999)), (1.0 + k) / (10.0 + k)))
        assert E.decay_of(state) == want and E.decay_of(state).dtype == np.float32
        _, state, dk = E.ema_ref(np.zeros(1), np.ones(1), state)
        assert dk == want
    assert E.decay_of(E.make_state(0.999, 10.0, 1, done=0)) == np.float32(2.0 / 11.0)
    assert E.decay_of(E.make_state(0.999, 10.0, 1, done=10 ** 6)) == np.float32(0.999)          # the cap
    assert E.decay_of(E.make_state(0.5, 0.0, 1, done=0)) == np.float32(0.5)


def test_restatement_every_third_step_updates():
    state = E.make_state(0.9, 0.0, 3)
    e, p = np.array([1.0]), np.array([0.0])
    updated = []
    for _ in range(7):
        e, state, d = E.ema_ref(e, p, state)
        updated.append(d is not None)
    assert updated == [False, False, True, False, False, True, False]
    assert state[E.I_SEEN] == 7 and state[E.I_DONE] == 2
    assert math.isclose(float(e[0]), float(np.float32(0.9)) ** 2, rel_tol=1e-15)


def test_restatement_skipped_step_leaves_everything_alone():
    state = E.make_state(0.9, 2.0, 1, seen=4, done=4)
    e, p = np.array([1.0, -2.0]), np.array([0.5, 0.25])
    for ss in (float("inf"), float("-inf"), float("nan")):
        assert E.overflowed(ss)
        e2, s2, d = E.ema_ref(e, p, state, sumsq=ss)
        assert d is None and np.array_equal(e2, e) and s2.tobytes() == state.tobytes()
    for ss in (0.0, 3.5, E.F64_MAX):
        assert not E.overflowed(ss)
        e2, s2, d = E.ema_ref(e, p, state, sumsq=ss)
        assert d is not None and not np.array_equal(e2, e) and s2[E.I_SEEN] == 5 and s2[E.I_DONE] == 5
    e3, s3, _ = E.ema_ref(e, p, state, sumsq=None)
    assert np.array_equal(e3, e2) and s3.tobytes() == s2.tobytes()


def test_geometry_comes_from_the_source_and_the_sizes_reach_every_path():
    c = E.kernel_constants()
    assert c["NT"] > 1 and c["U"] > 1 and c["GRID_CAP"] >= 1
    sizes = E.abi_sizes(c)
    chunk = c["U"] * c["NT"]
    assert E.grid_blocks(sizes[3], c) == 1 and sizes[3] % chunk == 0                       # exactly one full chunk
    assert E.grid_blocks(sizes[4], c) == 2 and sizes[4] % chunk == 3                       # a second block with a partial chunk
    big = sizes[-1]
    assert E.grid_blocks(big, c) == c["GRID_CAP"] and E.trips_of_block0(big, c) == 2 and big % chunk == 1
    assert E.trips_of_block0(big - 1, c) == 1                                              # the smallest such n
    # a partial chunk satisfies the issue bound only where results are normal: the subnormal values pair up as documented
    e, p = E.values("subnormal", 9)
    tiny = np.finfo(np.float32).tiny
    assert all((abs(a) < tiny) != (abs(b) < tiny) or a == b for a, b in zip(e, p))
    e, p = E.values("both_subnormal", 9)
    assert np.all(np.abs(e) < tiny) and np.all(np.abs(p) < tiny) and np.all(e != 0) and np.all(p != 0)


def test_model_state_dict_has_the_models_keys_and_the_shadows_values():
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True)
    frozen = next(n for n, p in model.named_parameters() if p.ndim > 1)
    dict(model.named_parameters())[frozen].requires_grad_(False)
    stub = types.SimpleNamespace(flat=FlatParams(model.parameters()))          # FlatParams is device-agnostic bookkeeping
    ema = WeightEMA(stub, 0.9, 0.0, 1)
    assert ema.shadow.numel() == sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert ema.shadow.data_ptr() != stub.flat.flat_p.data_ptr() and torch.equal(ema.shadow, stub.flat.flat_p)
    ema.shadow.mul_(0.5)
    live = {k: v.clone() for k, v in model.state_dict().items()}
    sd = ema.model_state_dict(model)
    assert list(sd.keys()) == list(live.keys())
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert frozen not in trainable and trainable
    for k, v in sd.items():
        assert v.shape == live[k].shape and v.dtype == live[k].dtype
        want = live[k] * 0.5 if k in trainable else live[k]
        assert torch.equal(v, want), k
    # clones: the result survives whatever happens to the shadow and the model afterwards
    keep = {k: v.clone() for k, v in sd.items()}
    ema.shadow.zero_()
    stub.flat.flat_p.add_(1.0)
    assert all(torch.equal(sd[k], keep[k]) for k in sd)
    model2 = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True)
    model2.load_state_dict(sd)                                                  # loads like any checkpoint
