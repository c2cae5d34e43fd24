"""CPU-only tests of the vector-target path: VectorNPZDataset against NPZSequenceDataset channel by channel, the channel maps of
the eight moves (against the composed generators, their inverses, and the physics of a gradient field), tta_affine in f64, and the
C ABI of the new entry points (symbols, struct size, argument contracts -- nothing is launched)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L

import vector_cases as VC

TRANSFORMS = ["asinh", "signed_log", None]


# ---------------------------------------------------------------------------------------------
# VectorNPZDataset against NPZSequenceDataset per channel
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("vector_host")
    X, Y = VC.write_npz(root / "vec.npz", N=5, T=2, C=2, Cy=3, H=6, W=7, seed=11)
    for c in range(3):
        np.savez(root / f"ch{c}.npz", X=X, Y=Y[:, :, c:c + 1])
    np.savez(root / "tied.npz", X=np.concatenate([X, X]), Y=np.concatenate([Y[:, :, 0:1], Y[:, :, 1:2]]))
    return root, X, Y


CONSTS = ("y_scale", "min_vel", "max_vel", "trans_min", "trans_max")
ARGSETS = {
    "percentiles": dict(lower_percentile=1.0, upper_percentile=97.5),
    "default percentiles": dict(),
    "explicit bounds": dict(min_y=-7.5, max_y=8.75),
    "explicit scale": dict(y_transform_scale=3.0, lower_percentile=2.0, upper_percentile=98.0),
    "no scale percentile": dict(y_transform_percentile=None, min_y=-20.0, max_y=20.0),
    "clip off": dict(clip_outliers=False, lower_percentile=5.0, upper_percentile=95.0),
}


@pytest.mark.parametrize("transform", TRANSFORMS, ids=str)
@pytest.mark.parametrize("args", sorted(ARGSETS))
def test_constants_and_items_equal_the_scalar_dataset_per_channel(files, args, transform):
    root, X, Y = files
    kw = dict(ARGSETS[args], y_transform=transform)
    vec = U.VectorNPZDataset(str(root / "vec.npz"), VC.AXES_UVW, **kw)
    assert isinstance(vec, U.NPZSequenceDataset) and len(vec) == 5 and vec.Cy == 3
    skw = dict(kw)
    skw.setdefault("min_y", None)                    # the vector class has no built-in bounds
    skw.setdefault("max_y", None)
    for c in range(3):
        one = U.NPZSequenceDataset(str(root / f"ch{c}.npz"), **skw)
        for name in CONSTS:
            arr = getattr(vec, name)
            assert arr.dtype == np.float64 and arr.shape == (3,)
            assert arr[c] == getattr(one, name), (name, c, arr[c], getattr(one, name))
        assert vec.x_max == one.x_max and vec.norm_const == one.norm_const and isinstance(vec.norm_const, float)
        for i in (0, 4):
            (x, y, m), (sx, sy, sm) = vec[i], one[i]
            assert tuple(y.shape) == (2, 3, 6, 7) and tuple(m.shape) == (2, 1, 6, 7) and y.dtype == torch.float32
            assert torch.equal(x, sx) and torch.equal(m, sm)
            assert y[:, c:c + 1].numpy().tobytes() == sy.numpy().tobytes(), (c, i)
    # the constants differ between u / v and w (else the per-channel path would prove nothing)
    if args == "percentiles":
        assert vec.trans_max[0] != vec.trans_max[2] and vec.y_scale[0] != vec.y_scale[2]


def test_per_channel_arguments(files):
    root, X, Y = files
    lo, hi, sc = (-9.0, -8.0, -2.0), (9.5, 8.5, 2.5), (4.0, 5.0, 1.5)
    vec = U.VectorNPZDataset(str(root / "vec.npz"), VC.AXES_UVW, min_y=lo, max_y=hi, y_transform_scale=sc)
    for c in range(3):
        one = U.NPZSequenceDataset(str(root / f"ch{c}.npz"), min_y=lo[c], max_y=hi[c], y_transform_scale=sc[c])
        assert all(getattr(vec, n)[c] == getattr(one, n) for n in CONSTS)
        assert vec[1][1][:, c:c + 1].numpy().tobytes() == one[1][1].numpy().tobytes()
    with pytest.raises(ValueError):
        U.VectorNPZDataset(str(root / "vec.npz"), VC.AXES_UVW, min_y=(-1.0, -2.0), max_y=1.0)


@pytest.mark.parametrize("transform", TRANSFORMS, ids=str)
def test_tie_horizontal_against_the_stacked_file(files, transform):
    root, X, Y = files
    kw = dict(lower_percentile=1.0, upper_percentile=99.0, y_transform=transform)
    vec = U.VectorNPZDataset(str(root / "vec.npz"), VC.AXES_UVW, tie_horizontal=True, **kw)
    both = U.NPZSequenceDataset(str(root / "tied.npz"), min_y=None, max_y=None, **kw)
    w = U.NPZSequenceDataset(str(root / "ch2.npz"), min_y=None, max_y=None, **kw)
    for name in CONSTS:
        assert getattr(vec, name)[0] == getattr(vec, name)[1] == getattr(both, name), name
        assert getattr(vec, name)[2] == getattr(w, name), name
    # items: channel 0 of item i is item i of the stacked file, channel 1 is item 5 + i
    for i in (0, 3):
        y = vec[i][1]
        assert y[:, 0:1].numpy().tobytes() == both[i][1].numpy().tobytes()
        assert y[:, 1:2].numpy().tobytes() == both[5 + i][1].numpy().tobytes()
    untied = U.VectorNPZDataset(str(root / "vec.npz"), VC.AXES_UVW, **kw)
    assert untied.trans_max[0] != untied.trans_max[1]


def test_denormalize_broadcasts_along_the_channel_dim(files):
    root, X, Y = files
    for transform in TRANSFORMS:
        vec = U.VectorNPZDataset(str(root / "vec.npz"), VC.AXES_UVW, lower_percentile=1.0, upper_percentile=99.0, y_transform=transform)
        ones = [U.NPZSequenceDataset(str(root / f"ch{c}.npz"), min_y=None, max_y=None, lower_percentile=1.0, upper_percentile=99.0,
                                     y_transform=transform) for c in range(3)]
        y = torch.stack([vec[i][1] for i in range(5)])                       # [5, 2, 3, 6, 7]
        for arr in (y, y.double(), y.numpy(), y.double().numpy()):
            got = vec.denormalize(arr)
            assert type(got) is type(arr) and got.dtype == arr.dtype and tuple(got.shape) == tuple(arr.shape)
            for c in range(3):
                want = ones[c].denormalize(arr[:, :, c:c + 1])
                np.testing.assert_allclose(np.asarray(got[:, :, c:c + 1]), np.asarray(want), rtol=1e-5, atol=1e-5)
        with pytest.raises(ValueError):
            vec.denormalize(y[:, :, :2])


def test_bad_datasets_and_scalar_code_fail_loudly(files, tmp_path):
    root, X, Y = files
    path = str(root / "vec.npz")
    for axes in (("+w", "-h"), ("+w", "+w", None), ("+h", "-h", None), ("+w", "x", None), ("+w", "-h", None, None)):
        with pytest.raises(ValueError):
            U.VectorNPZDataset(path, axes)
    np.savez(tmp_path / "five.npz", X=X, Y=np.concatenate([Y, Y[:, :, :2]], axis=2))
    with pytest.raises(ValueError):
        U.VectorNPZDataset(str(tmp_path / "five.npz"), (None,) * 5)
    vec = U.VectorNPZDataset(path, VC.AXES_UVW)
    with pytest.raises(TypeError):
        float(vec.y_scale)                                                  # what every scalar consumer does first
    with pytest.raises(TypeError):
        vec._fwd(np.zeros(3))
    with pytest.raises(TypeError, match="vector"):
        U.EvalReport(vec, device="cpu")
    with pytest.raises(TypeError, match="vector"):
        U.evaluate_report(None, [], "cpu", vec)
    # Subset / random_split / the loader's root walk accept it
    sub = torch.utils.data.Subset(torch.utils.data.Subset(vec, [4, 2, 0]), [2, 0])
    from unet_convlstm_amd import engine as E
    r, rows = E._root_rows(sub)
    assert r is vec and rows.tolist() == [0, 4]
    assert [int(b[0]) for b in U.epoch_rows(sub, None, 1)] == [0, 4]
    with pytest.raises(U.UclstmError):
        U.DeviceSequenceLoader(vec, 2, device="cpu")


# ---------------------------------------------------------------------------------------------
# channel maps
# ---------------------------------------------------------------------------------------------
AXES_SETS = [VC.AXES_UVW, ("+w", "+h"), ("-w", "+h", None, None), (None, "-h", "-w"), (None,), (None, None), ("+h", None, "+w", None)]


def _ds(tmp_path, axes, S=4, **kw):
    rng = np.random.default_rng(len(axes))
    np.savez(tmp_path / "a.npz", X=(rng.random((2, 1, 2, S, S)) * 30).astype(np.float32),
             Y=rng.normal(0, 3, (2, 1, len(axes), S, S)).astype(np.float32))
    return U.VectorNPZDataset(str(tmp_path / "a.npz"), axes, **kw)


@pytest.mark.parametrize("axes", AXES_SETS, ids=str)
def test_channel_map_is_the_composition_of_the_generators_and_inverts(tmp_path, axes):
    ds = _ds(tmp_path, axes)
    ident = [(c, False) for c in range(len(axes))]
    tab = ds.chan_map_table()
    assert tab.dtype == np.int8 and tab.shape == (8, len(axes))
    for code in range(8):
        cm = ds.channel_map(code)
        assert cm == VC.generator_map(axes, code), code
        back = ds.channel_map(U.d4_inverse(code))
        assert [(cm[src][0], cm[src][1] != neg) for src, neg in back] == ident, code          # inverse after the move
        assert [int(v) & 7 for v in tab[code]] == [s for s, _ in cm] and [bool(int(v) & 0x80) for v in tab[code]] == [n for _, n in cm]
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            ds.channel_map(bad)


def test_the_uvw_example_by_hand(tmp_path):
    ds = _ds(tmp_path, VC.AXES_UVW)
    assert ds.channel_map(0) == [(0, False), (1, False), (2, False)]
    assert ds.channel_map(1) == [(0, True), (1, False), (2, False)]          # mirror left-right: u changes sign
    assert ds.channel_map(2) == [(0, False), (1, True), (2, False)]          # mirror up-down: v changes sign
    assert ds.channel_map(4) == [(1, True), (0, True), (2, False)]           # transpose: u' = -v^T, v' = -u^T
    same = _ds(tmp_path, ("+w", "+h", None))
    assert same.channel_map(4) == [(1, False), (0, False), (2, False)]


@pytest.mark.parametrize("axes", [("+w", None), (None, "-h"), ("+h",)], ids=str)
def test_a_transpose_with_one_horizontal_channel_is_refused(tmp_path, axes):
    ds = _ds(tmp_path, axes)
    for code in range(4):
        assert ds.channel_map(code) == VC.generator_map(axes, code)
    for code in range(4, 8):
        with pytest.raises(ValueError):
            ds.channel_map(code)
        assert [int(v) for v in ds.chan_map_table()[code]] == list(range(len(axes)))


@pytest.mark.parametrize("axes", [VC.AXES_UVW, ("+w", "+h"), ("-h", None, "-w"), ("-w", "+h", None, None)], ids=str)
@pytest.mark.parametrize("code", range(8))
def test_the_gradient_field_of_a_moved_potential_is_the_moved_field(tmp_path, axes, code):
    """The physics, with no reference to channel_map's rules (vector_cases.potential_field): exact in integers."""
    S = 12
    ds = _ds(tmp_path, axes)
    field = torch.from_numpy(VC.potential_field(axes, S, 0))
    want = torch.from_numpy(VC.potential_field(axes, S, code))
    got = VC.apply_map(field, code, ds.channel_map(code))
    assert torch.equal(got, want), f"axes {axes} code {code}: {int((got != want).sum())} values differ"
    assert float(field.float().double().sub(field.double()).abs().max()) == 0.0          # exactly representable in f32
    if code:
        assert not torch.equal(VC.torch_move(field, code), want)                          # the planes alone are not enough


# ---------------------------------------------------------------------------------------------
# tta_affine
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", TRANSFORMS, ids=str)
def test_tta_affine_maps_normalised_fields_in_f64(files, tmp_path, transform):
    root, X, Y = files
    rng = np.random.default_rng(3)
    np.savez(tmp_path / "sq.npz", X=(rng.random((3, 2, 2, 6, 6)) * 30).astype(np.float32),
             Y=(rng.standard_normal((3, 2, 3, 6, 6)) * np.array([9.0, 7.0, 2.0]).reshape(1, 1, 3, 1, 1)).astype(np.float32))
    ds = U.VectorNPZDataset(str(tmp_path / "sq.npz"), VC.AXES_UVW, tie_horizontal=True, clip_outliers=False, lower_percentile=1.0,
                            upper_percentile=99.0, y_transform=transform)
    raw = torch.from_numpy(ds.Y).double()
    norm = torch.from_numpy(VC.normalise64(ds.Y, ds))
    for code in range(8):
        want = torch.from_numpy(VC.normalise64(VC.apply_map(raw, code, ds.channel_map(code)).numpy(), ds))
        aff = ds.tta_affine(code)
        assert [(s, sign < 0) for s, sign, _ in aff] == ds.channel_map(code)
        got = VC.apply_affine(norm, code, aff)
        err = float((got - want).abs().max())
        assert err <= 1e-12, (code, err)
    untied = U.VectorNPZDataset(str(tmp_path / "sq.npz"), VC.AXES_UVW, clip_outliers=False, y_transform=transform)
    for code in range(4):
        untied.tta_affine(code)                                             # mirrors need no shared constants
    for code in range(4, 8):
        with pytest.raises(ValueError, match="tie_horizontal"):
            untied.tta_affine(code)
    with pytest.raises(ValueError, match="tie_horizontal"):
        U.predict_tta(lambda x: (x, None), torch.zeros(1, 1, 3, 4, 4), "d4", dataset=untied)        # before any launch
    with pytest.raises(TypeError):
        U.predict_tta(lambda x: (x, None), torch.zeros(1, 1, 3, 4, 4), "flips", dataset=U.NPZSequenceDataset(str(root / "ch0.npz")))


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
NEW = {"uclstm_dataset_gather_vec": 24, "uclstm_plane_d4_vec": 12, "uclstm_loss_spec_fwd_bc": 10, "uclstm_loss_spec_fwd_ordered_bc": 12,
       "uclstm_loss_spec_bwd_bc": 11, "uclstm_metric_sums_vec": 12, "uclstm_metric_sums_vec_rows": 3}


def test_the_new_entry_points_are_in_the_header_the_binding_and_the_library():
    hdr = open(L.HEADER_PATH).read()
    raw = C.CDLL(L.LIB_PATH)
    for sym, arity in NEW.items():
        assert sym in L._PROTOS and sym in L.header_symbols() and hasattr(raw, sym), sym
        assert not hasattr(raw, sym + "_f16")
        params = re.search(r"\b%s\s*\(([^)]*)\)" % sym, hdr).group(1)
        params = re.sub(r"/\*.*?\*/", "", params, flags=re.S)
        assert len([a for a in params.split(",") if a.strip()]) == len(L._PROTOS[sym]) == arity, sym
    assert C.sizeof(L.TargetConsts) == 20
    assert re.search(r"#define UCLSTM_VEC_MAX\s+4\b", hdr) and L.VEC_MAX == 4
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16            # additive change
    assert int(re.search(r"#define UCLSTM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 16
    for name in ("VectorNPZDataset", "plane_d4_vec"):
        assert name in U.__all__ and hasattr(U, name)


def _consts(n=4, **over):
    vals = dict(min_vel=-7.5, max_vel=8.5, y_scale=2.0, trans_min=-2.0, trans_max=2.2)
    arr = (L.TargetConsts * n)(*[L.TargetConsts(**vals) for _ in range(n)])
    for k, v in over.items():
        setattr(arr[n - 1], k, v)                                           # the LAST channel: every channel is validated
    return arr


VEC_ORDER = ("x_all", "y_all", "idx", "aug", "n_seq", "n_out", "T_src", "T_out", "C", "Cy", "Hs", "Ws", "Ho", "Wo", "flags", "chan_map",
             "x", "y", "mask", "transform", "norm_const", "clip", "consts")


def _vec_args(**over):
    """Arguments that pass validation (the data pointers are garbage, 16-byte aligned: a call that accepted them would launch)."""
    consts = over.pop("consts", "default")
    a = dict(x_all=0x1000, y_all=0x2000, idx=0x3000, aug=0x7000, n_seq=8, n_out=4, T_src=4, T_out=3, C=2, Cy=3, Hs=16, Ws=16, Ho=8, Wo=8,
             flags=3, chan_map=None, x=0x4000, y=0x5000, mask=0x6000, transform=1, norm_const=30.0, clip=1)
    assert set(over) <= set(a)
    a.update(over)
    a["consts"] = _consts(max(1, min(a["Cy"], 4))) if consts == "default" else consts
    return [a[k] for k in VEC_ORDER] + [None]


VEC_BAD = {
    "null x_all": dict(x_all=None), "null y_all": dict(y_all=None), "null x": dict(x=None), "null y": dict(y=None),
    "null mask": dict(mask=None), "null consts": dict(consts=None),
    "Cy = 0": dict(Cy=0), "Cy < 0": dict(Cy=-1), "Cy = 5": dict(Cy=5),
    "n_seq = 0": dict(n_seq=0), "n_out = 0": dict(n_out=0), "T_out = 0": dict(T_out=0), "C = 0": dict(C=0), "Hs = 0": dict(Hs=0),
    "Ho > Hs": dict(Ho=17, Wo=16, flags=2), "Wo > Ws": dict(Ho=16, Wo=17, flags=2), "T_out > T_src": dict(T_out=5),
    "t allowed but Ho != Wo": dict(Ho=8, Wo=4, flags=1), "unknown flag bits": dict(flags=4), "negative flags": dict(flags=-1),
    "transform 3": dict(transform=3), "transform -1": dict(transform=-1), "norm_const = 0": dict(norm_const=0.0),
    "asinh with y_scale = 0 in the last channel": dict(transform=1, consts=_consts(3, y_scale=0.0)),
    "signed_log with y_scale < 0": dict(transform=2, consts=_consts(3, y_scale=-1.0)),
    "trans_max == trans_min": dict(consts=_consts(3, trans_max=-2.0)),
    "identity index with n_out > n_seq": dict(idx=None, n_out=9),
    "2^31 target pixels only with Cy": dict(n_seq=1 << 20, n_out=1 << 14, T_src=1 << 4, T_out=1 << 4, Hs=64, Ws=64, Ho=64, Wo=64, Cy=2),
    "a source frame of 2^31 pixels only with Cy": dict(Hs=1 << 15, Ws=1 << 15, Cy=2),
}


@pytest.mark.parametrize("name", sorted(VEC_BAD))
def test_gather_vec_rejects_bad_arguments_before_any_launch(name):
    # no GPU here and the data pointers are garbage: anything but an early UCLSTM_E_BADARG would be a launch error (-2) or a crash
    assert L.lib.uclstm_dataset_gather_vec(*_vec_args(**VEC_BAD[name])) == -1, name


def _plane_args(**over):
    a = dict(src=0x1000, dst=0x2000, n_frames=6, Cy=3, H=8, W=12, code=5, chan_map=None, offset=None, accumulate=0, scale=1.0)
    assert set(over) <= set(a)
    a.update(over)
    return [a[k] for k in ("src", "dst", "n_frames", "Cy", "H", "W", "code", "chan_map", "offset", "accumulate", "scale")] + [None]


PLANE_BAD = {
    "null src": dict(src=None), "null dst": dict(dst=None), "n_frames = 0": dict(n_frames=0), "n_frames < 0": dict(n_frames=-2),
    "Cy = 0": dict(Cy=0), "Cy = 5": dict(Cy=5), "H = 0": dict(H=0), "W < 0": dict(W=-1), "code 8": dict(code=8), "code -1": dict(code=-1),
    "2^31 elements only with Cy": dict(n_frames=1 << 10, Cy=2, H=1 << 10, W=1 << 10),
    "a frame of 2^31 elements only with Cy": dict(n_frames=1, Cy=2, H=1 << 15, W=1 << 15),
}


@pytest.mark.parametrize("name", sorted(PLANE_BAD))
def test_plane_d4_vec_rejects_bad_arguments_before_any_launch(name):
    assert L.lib.uclstm_plane_d4_vec(*_plane_args(**PLANE_BAD[name])) == -1, name


def test_loss_bc_and_metric_vec_reject_bad_arguments_before_any_launch():
    spec = L.LossSpecDesc(L.LOSS_POINT_L1, 3, 1.0, 4.0, 1)
    ok = dict(yp=0x1000, y=0x2000, mask=0x3000, out=0x4000, planes=6, H=8, W=8, div=3)
    for over in (dict(mask=None), dict(div=0), dict(div=-3), dict(yp=None), dict(out=None), dict(planes=0), dict(H=0), dict(planes=1 << 20, H=64, W=64)):
        a = dict(ok, **over)
        assert L.lib.uclstm_loss_spec_fwd_bc(C.byref(spec), a["yp"], a["y"], a["mask"], a["out"], a["planes"], a["H"], a["W"], a["div"], None) == -1, over
        assert L.lib.uclstm_loss_spec_fwd_ordered_bc(C.byref(spec), a["yp"], a["y"], a["mask"], 0x5000, a["out"], 0, a["planes"], a["H"],
                                                     a["W"], a["div"], None) == -1, over
        assert L.lib.uclstm_loss_spec_bwd_bc(C.byref(spec), a["yp"], a["y"], a["mask"], 0x5000, a["out"], a["planes"], a["H"], a["W"],
                                             a["div"], None) == -1, over
    assert L.lib.uclstm_loss_spec_fwd_bc(None, 0x1000, 0x2000, 0x3000, 0x4000, 6, 8, 8, 3, None) == -1
    k = _consts(3)
    good = dict(yp=0x1000, y=0x2000, mask=None, partials=0x3000, sums=0x4000, acc=0, n=6, Cy=3, HW=64, tr=1, consts=k)
    for over in (dict(yp=None), dict(y=None), dict(partials=None), dict(sums=None), dict(consts=None), dict(n=0), dict(Cy=0), dict(Cy=5),
                 dict(HW=0), dict(tr=3), dict(tr=-1), dict(n=1 << 20, HW=1 << 10)):
        a = dict(good, **over)
        assert L.lib.uclstm_metric_sums_vec(a["yp"], a["y"], a["mask"], a["partials"], a["sums"], a["acc"], a["n"], a["Cy"], a["HW"],
                                            a["tr"], a["consts"], None) == -1, over
    assert L.lib.uclstm_metric_sums_vec_rows(6, 3, 64) == 2 and L.lib.uclstm_metric_sums_vec_rows(6, 5, 64) == -1
    assert L.lib.uclstm_metric_sums_vec_rows(1 << 20, 1, 64 * 64) == -1 and L.lib.uclstm_metric_sums_vec_rows(1 << 12, 1, 64 * 64) == 1024
