"""CPU-only tests of on-device augmentation: the epoch table (epoch_augment), the code algebra (index formula, inverse rule)
against torch, and the C ABI of uclstm_dataset_gather_augment / uclstm_plane_d4 (symbols, argument contract -- nothing is
launched)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L

GATHER, PLANE = "uclstm_dataset_gather_augment", "uclstm_plane_d4"


def _G(seed):
    return torch.Generator().manual_seed(seed)


def torch_move(s, code):
    """The meaning of a code, as the issue states it."""
    if code & 1:
        s = s.flip(-1)
    if code & 2:
        s = s.flip(-2)
    if code & 4:
        s = s.transpose(-2, -1)
    return s


def inv(c):
    return c if not c & 4 else 4 | (c & 1) << 1 | (c & 2) >> 1


# ---------------------------------------------------------------------------------------------
# epoch_augment
# ---------------------------------------------------------------------------------------------
def test_a_seed_reproduces_the_table_and_another_seed_does_not():
    aug = U.Augment(hflip=True, vflip=True, transpose=True, crop=(16, 16), frames=3, crop_align=4)
    a, b = U.epoch_augment(64, 5, 40, 40, aug, _G(3)), U.epoch_augment(64, 5, 40, 40, aug, _G(3))
    c = U.epoch_augment(64, 5, 40, 40, aug, _G(4))
    assert a.dtype == np.int32 and a.shape == (64, 4) and np.array_equal(a, b) and not np.array_equal(a, c)
    # one generator, two epochs: the stream continues
    g = _G(3)
    first, second = U.epoch_augment(64, 5, 40, 40, aug, g), U.epoch_augment(64, 5, 40, 40, aug, g)
    assert np.array_equal(first, a) and not np.array_equal(second, a)
    # the documented order: all codes, then all oy, then all ox, then all t0
    g = _G(3)
    want = [torch.randint(0, n, (64,), generator=g).numpy() for n in (8, 7, 7, 3)]
    assert np.array_equal(a[:, 0], want[0]) and np.array_equal(a[:, 1], want[1] * 4)
    assert np.array_equal(a[:, 2], want[2] * 4) and np.array_equal(a[:, 3], want[3])


def test_codes_cover_the_group_and_respect_the_enabled_bits():
    full = U.epoch_augment(4096, 4, 8, 8, U.Augment(hflip=True, vflip=True, transpose=True), _G(0))
    assert set(full[:, 0].tolist()) == set(range(8))
    assert not full[:, 1:].any()                                         # no crop, no time window: zero
    only_h = U.epoch_augment(4096, 4, 8, 8, U.Augment(hflip=True), _G(0))
    assert set(only_h[:, 0].tolist()) == {0, 1} and not only_h[:, 1:].any()
    only_vt = U.epoch_augment(4096, 4, 8, 8, U.Augment(vflip=True, transpose=True), _G(0))
    assert set(only_vt[:, 0].tolist()) == {0, 2, 4, 6}
    none = U.epoch_augment(100, 4, 8, 8, U.Augment(), _G(0))
    assert none.shape == (100, 4) and not none.any()
    assert U.epoch_augment(0, 4, 8, 8, U.Augment(hflip=True), _G(0)).shape == (0, 4)


@pytest.mark.parametrize("align", [1, 3, 4])
def test_windows_stay_inside_the_source_on_the_alignment_grid(align):
    T, H, W, Ho, Wo, To = 6, 40, 37, 16, 9, 4
    tab = U.epoch_augment(4096, T, H, W, U.Augment(crop=(Ho, Wo), frames=To, crop_align=align), _G(1))
    assert not tab[:, 0].any()
    for col, size, out in ((1, H, Ho), (2, W, Wo)):
        v = tab[:, col]
        assert v.min() >= 0 and v.max() + out <= size and not (v % align).any()
        assert set(v.tolist()) == set(range(0, size - out + 1, align))    # every valid position occurs in 4096 draws
    assert set(tab[:, 3].tolist()) == set(range(T - To + 1))


def test_bad_configurations_raise():
    with pytest.raises(ValueError):
        U.Augment(transpose=True, crop=(8, 4))
    with pytest.raises(ValueError):
        U.epoch_augment(4, 2, 5, 7, U.Augment(transpose=True), _G(0))     # full frame, not square
    with pytest.raises(ValueError):
        U.epoch_augment(4, 2, 8, 8, U.Augment(crop=(9, 8)), _G(0))
    with pytest.raises(ValueError):
        U.epoch_augment(4, 2, 8, 8, U.Augment(frames=3), _G(0))
    with pytest.raises(ValueError):
        U.Augment(crop=(0, 4))
    with pytest.raises(ValueError):
        U.Augment(crop_align=0)
    with pytest.raises(Exception):
        U.Augment().hflip = True                                          # frozen


# ---------------------------------------------------------------------------------------------
# the codes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", range(8))
def test_index_formula_and_inverse_rule_against_torch(code):
    s = torch.arange(15.0).reshape(3, 5)
    Hc, Wc = s.shape
    out = torch_move(s, code)
    assert tuple(out.shape) == ((Wc, Hc) if code & 4 else (Hc, Wc))
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            a, b = (j, i) if code & 4 else (i, j)
            if code & 2:
                a = Hc - 1 - a
            if code & 1:
                b = Wc - 1 - b
            assert out[i, j] == s[a, b], (code, i, j)
    assert U.d4_inverse(code) == inv(code)
    assert torch.equal(torch_move(out, inv(code)), s)
    # the eight codes are eight distinct moves
    sq = torch.arange(16.0).reshape(4, 4)
    assert sum(torch.equal(torch_move(sq, code), torch_move(sq, other)) for other in range(8)) == 1


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def test_both_entry_points_are_in_the_header_the_binding_and_the_library():
    hdr = open(L.HEADER_PATH).read()
    raw = C.CDLL(L.LIB_PATH)
    for sym, arity in ((GATHER, 26), (PLANE, 9)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert sym in L._PROTOS and sym in L.header_symbols() and hasattr(raw, sym)
        assert sym not in L.F16_TWINS and not hasattr(raw, sym + "_f16")
        params = re.search(r"\b%s\s*\(([^)]*)\)" % sym, hdr).group(1)
        params = re.sub(r"/\*.*?\*/", "", params, flags=re.S)
        assert len([a for a in params.split(",") if a.strip()]) == len(L._PROTOS[sym]) == arity
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16            # additive change
    assert int(re.search(r"#define UCLSTM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 16
    for name in ("Augment", "epoch_augment", "plane_d4", "predict_tta", "d4_inverse"):
        assert name in U.__all__ and hasattr(U, name)


GATHER_ORDER = ("x_all", "y_all", "idx", "aug", "n_seq", "n_out", "T_src", "T_out", "C", "Hs", "Ws", "Ho", "Wo", "flags", "x", "y",
                "mask", "transform", "norm_const", "min_vel", "max_vel", "clip", "y_scale", "trans_min", "trans_max")


def _gather_args(**over):
    """Arguments that pass validation (the pointers are garbage, 16-byte aligned: a call that accepted them would launch)."""
    a = dict(x_all=0x1000, y_all=0x2000, idx=0x3000, aug=0x7000, n_seq=8, n_out=4, T_src=4, T_out=3, C=2, Hs=16, Ws=16, Ho=8, Wo=8,
             flags=3, x=0x4000, y=0x5000, mask=0x6000, transform=1, norm_const=30.0, min_vel=-7.5, max_vel=8.5, clip=1, y_scale=2.0,
             trans_min=-2.0, trans_max=2.2)
    assert set(over) <= set(a)
    a.update(over)
    return [a[k] for k in GATHER_ORDER] + [None]


GATHER_BAD = {
    "null x_all": dict(x_all=None), "null y_all": dict(y_all=None), "null aug": dict(aug=None), "null x": dict(x=None),
    "null y": dict(y=None), "null mask": dict(mask=None),
    "n_seq = 0": dict(n_seq=0), "n_seq < 0": dict(n_seq=-1), "n_out = 0": dict(n_out=0), "n_out < 0": dict(n_out=-3),
    "T_src = 0": dict(T_src=0, T_out=0), "T_out = 0": dict(T_out=0), "T_out < 0": dict(T_out=-1), "C = 0": dict(C=0), "C < 0": dict(C=-2),
    "Hs = 0": dict(Hs=0), "Ws < 0": dict(Ws=-16), "Ho = 0": dict(Ho=0, flags=2), "Wo = 0": dict(Wo=0, flags=2), "Ho < 0": dict(Ho=-8, flags=2),
    "Ho > Hs": dict(Ho=17, Wo=16, flags=2), "Wo > Ws": dict(Ho=16, Wo=17, flags=2), "square but too large": dict(Ho=17, Wo=17),
    "T_out > T_src": dict(T_out=5),
    "t allowed but Ho != Wo": dict(Ho=8, Wo=4, flags=1), "t allowed but Ho != Wo, aligned": dict(Ho=4, Wo=8, flags=3),
    "unknown flag bits": dict(flags=4), "negative flags": dict(flags=-1),
    "transform 3": dict(transform=3), "transform -1": dict(transform=-1),
    "norm_const = 0": dict(norm_const=0.0), "trans_max == trans_min": dict(trans_max=-2.0),
    "asinh with y_scale = 0": dict(transform=1, y_scale=0.0), "signed_log with y_scale < 0": dict(transform=2, y_scale=-1.0),
    "identity index with n_out > n_seq": dict(idx=None, n_out=9),
    "2^31 pixels": dict(n_seq=1 << 20, n_out=1 << 15, T_src=1 << 4, T_out=1 << 4, Hs=64, Ws=64, Ho=64, Wo=64),
    "beyond 2^31 pixels": dict(n_seq=1 << 40, n_out=1 << 40, T_src=1 << 20, T_out=1 << 20, Hs=1 << 10, Ws=1 << 10, Ho=1 << 10, Wo=1 << 10),
    "a source frame of 2^31 pixels": dict(Hs=1 << 16, Ws=1 << 15),
}


@pytest.mark.parametrize("name", sorted(GATHER_BAD))
def test_gather_augment_rejects_bad_arguments_before_any_launch(name):
    # no GPU here and the pointers are garbage: anything but an early UCLSTM_E_BADARG would be a launch error (-2) or a crash
    assert L.lib.uclstm_dataset_gather_augment(*_gather_args(**GATHER_BAD[name])) == -1, name


def _plane_args(**over):
    a = dict(src=0x1000, dst=0x2000, n_planes=6, H=8, W=12, code=5, accumulate=0, scale=1.0)
    assert set(over) <= set(a)
    a.update(over)
    return [a[k] for k in ("src", "dst", "n_planes", "H", "W", "code", "accumulate", "scale")] + [None]


PLANE_BAD = {
    "null src": dict(src=None), "null dst": dict(dst=None), "n_planes = 0": dict(n_planes=0), "n_planes < 0": dict(n_planes=-2),
    "H = 0": dict(H=0), "H < 0": dict(H=-8), "W = 0": dict(W=0), "W < 0": dict(W=-1),
    "code 8": dict(code=8), "code -1": dict(code=-1), "code 13": dict(code=13),
    "2^31 elements": dict(n_planes=1 << 11, H=1 << 10, W=1 << 10), "a plane of 2^31 elements": dict(n_planes=1, H=1 << 16, W=1 << 15),
}


@pytest.mark.parametrize("name", sorted(PLANE_BAD))
def test_plane_d4_rejects_bad_arguments_before_any_launch(name):
    assert L.lib.uclstm_plane_d4(*_plane_args(**PLANE_BAD[name])) == -1, name


# ---------------------------------------------------------------------------------------------
# host layer without a GPU
# ---------------------------------------------------------------------------------------------
def test_the_loader_with_augment_still_needs_a_device(tmp_path):
    rng = np.random.default_rng(5)
    np.savez(tmp_path / "ds.npz", X=(rng.random((4, 2, 2, 4, 4)) * 30).astype(np.float32),
             Y=rng.normal(0, 3, (4, 2, 1, 4, 4)).astype(np.float32))
    ds = U.NPZSequenceDataset(str(tmp_path / "ds.npz"))
    with pytest.raises(U.UclstmError):
        U.DeviceSequenceLoader(ds, 2, device="cpu", augment=U.Augment(hflip=True))
    with pytest.raises(U.UclstmError):
        U.plane_d4(torch.zeros(2, 4, 4), 1)                               # no CPU path
    with pytest.raises(ValueError):
        U.predict_tta(lambda x: (x, None), torch.zeros(1, 1, 1, 3, 5), "d4")          # t on a non-square input
    with pytest.raises(ValueError):
        U.predict_tta(lambda x: (x, None), torch.zeros(1, 1, 1, 4, 4), "rotations")
    with pytest.raises(ValueError):
        U.predict_tta(lambda x: (x, None), torch.zeros(1, 1, 1, 4, 4), (0, 8))
