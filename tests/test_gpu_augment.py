"""GPU tests of on-device augmentation.  uclstm_dataset_gather_augment is checked BIT FOR BIT against the existing
uclstm_dataset_gather_transform output of the same rows moved with torch.flip / transpose / slicing (the remap commutes with the
per-pixel arithmetic, so no tolerance is needed): 16-byte and scalar paths, partial LDS tiles, non-square frames, the run-time
channel loop, the time window, clamping of a bad table; then DeviceSequenceLoader(augment=...), plane_d4, predict_tta and
evaluate(tta=...)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, sub

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import engine as E

DEV = "cuda"
X_TOL = dict(rtol=1e-6, atol=1e-7)          # tests/test_gpu_device_loader.py
Y_TOL = dict(rtol=1e-5, atol=2e-6)          # tests/test_gpu_device_loader.py (asinh)
TRANSFORMS = ["asinh", "signed_log", None]


def torch_move(s, code):
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
# data
# ---------------------------------------------------------------------------------------------
SHAPES = {"40": (3, 2, 2, 40, 40), "5x7": (5, 1, 2, 5, 7), "c4": (4, 3, 4, 4, 8), "12": (10, 3, 2, 12, 12)}


def _raw(case):
    if case == "golden":                                                   # N = 3, T = 4, C = 2, 8 x 8
        g = load_golden("dataset")
        X, Y = g["X"].numpy().copy(), g["Y"].numpy().copy()
    else:
        rng = np.random.default_rng(len(case) + 40)
        N, T, C, H, W = SHAPES[case]
        X = (rng.random((N, T, C, H, W)) * 40).astype(np.float32)
        X[X < 8] = 0.0
        Y = (rng.standard_normal((N, T, 1, H, W)) * 3).astype(np.float32)
    # the values at which the arithmetic can go wrong: raw channel 0 around float32(1.1), targets outside the clip range, zeros
    t = np.float32(1.1)
    X[0, 0, 0].reshape(-1)[:3] = [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(2))]
    X[-1, -1, 0].reshape(-1)[-3:] = X[0, 0, 0].reshape(-1)[:3]
    Y.reshape(-1)[:6] = [-20.0, 15.0, 0.0, -0.0, -7.6, 8.79]
    Y.reshape(-1)[-4:] = [0.0, 40.0, -30.0, 1e-30]
    return X, Y


_cache = {}


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(case, transform, clip) -> (dataset, x_all, y_all on the device, the PLAIN kernel's output for every row in order);
    built once, never changed."""
    root = tmp_path_factory.mktemp("augment")

    def get(case, transform="asinh", clip=True):
        key = (case, transform, clip)
        if key not in _cache:
            path = root / f"{case}.npz"
            if not path.exists():
                X, Y = _raw(case)
                np.savez(path, X=X, Y=Y)
            ds = U.NPZSequenceDataset(str(path), y_transform=transform, clip_outliers=clip)
            xa, ya = torch.from_numpy(ds.X).to(DEV), torch.from_numpy(ds.Y).to(DEV)
            _cache[key] = (ds, xa, ya, E._gather_transform(ds, xa, ya, None, len(ds)))
        return _cache[key]
    return get


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(-1, 4)


def _moved(plain, idx, tab, shape):
    """The plain kernel's rows ``idx`` moved as the table says, with torch alone."""
    To, Ho, Wo = shape
    out = []
    for t in plain:
        seqs = []
        for row, (code, oy, ox, t0) in zip(idx, tab):
            Hc, Wc = (Wo, Ho) if code & 4 else (Ho, Wo)
            seqs.append(torch_move(t[row, t0:t0 + To, :, oy:oy + Hc, ox:ox + Wc], code))
        out.append(torch.stack(seqs))
    return out


def _run_and_compare(made_case, idx, tab, shape, flags, what):
    ds, xa, ya, plain = made_case
    got = E._gather_augment(ds, xa, ya, torch.tensor(idx, dtype=torch.int64, device=DEV), _table(tab), len(idx), shape, flags)
    want = _moved(plain, idx, tab, shape)
    C = xa.shape[2]
    for g, w, name, ch in zip(got, want, ("x", "y", "mask"), (C, 1, 1)):
        assert tuple(g.shape) == (len(idx), shape[0], ch, shape[1], shape[2]) and g.is_contiguous(), (what, name)
        assert torch.equal(g, w), f"{what}: {name} differs in {int((g != w).sum())} of {g.numel()} elements"
    return got


# ---------------------------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------------------------
IDX8 = [2, 0, 2, 1, 0, 2, 1, 1]                    # a duplicate, out of order; position k carries code k


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("transform", TRANSFORMS)
def test_full_frame_all_codes_16_byte_path(made, transform, clip):
    case = made("golden", transform, clip)
    tab = [[k, 0, 0, 0] for k in range(8)]
    x, y, m = _run_and_compare(case, IDX8, tab, (4, 8, 8), 3, f"golden {transform} clip={clip}")
    if transform == "asinh" and clip:
        # ... and against the host dataset moved the same way, so that the check does not rest on the old kernel alone
        ds = case[0]
        for k, row in enumerate(IDX8):
            hx, hy, hm = (torch_move(t, k) for t in ds[row])
            torch.testing.assert_close(x[k].cpu(), hx, **X_TOL)
            torch.testing.assert_close(y[k].cpu(), hy, **Y_TOL)
            assert torch.equal(m[k].cpu(), hm)


@pytest.mark.parametrize("crop,oy,ox,flags", [(36, 1, 3, 1), (36, 4, 4, 3), (33, 7, 0, 3), (33, 7, 0, 1)])
def test_partial_tiles_in_both_dimensions(made, crop, oy, ox, flags):
    """40 x 40 source: 36 x 36 is 2 x 2 LDS tiles with a partial last row and column of tiles; (1, 3) takes the scalar path (ox is
    no multiple of 4), (4, 4) the 16-byte path; 33 x 33 is an odd width: scalar path, a ragged last tile of one pixel (the flag
    for aligned offsets alone must not select the 16-byte path)."""
    tab = [[k, oy, ox, 0] for k in range(8)]
    _run_and_compare(made("40"), [0, 1, 2, 0, 1, 2, 0, 1], tab, (2, crop, crop), flags, f"40 crop {crop} at ({oy}, {ox})")


def test_non_square_frames_take_the_codes_without_t(made):
    case = made("5x7")
    ds, xa, ya, _ = case
    _run_and_compare(case, [4, 0, 3, 3, 1], [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [3, 0, 0, 0], [3, 0, 0, 0]], (1, 5, 7), 0, "5x7")
    _run_and_compare(case, [2, 1, 0, 4], [[k, 1, 2, 0] for k in range(4)], (1, 3, 4), 0, "5x7 crop 3x4")
    with pytest.raises(U.UclstmError):                                     # a table that may hold t needs Ho == Wo
        E._gather_augment(ds, xa, ya, None, _table([[4, 0, 0, 0]]), 1, (1, 5, 7), 1)


@pytest.mark.parametrize("ox,flags", [([0, 4, 2, 4, 0, 1, 3, 4], 1), ([0, 4, 4, 0, 4, 0, 0, 4], 3)])
def test_run_time_channel_loop(made, ox, flags):
    tab = [[k, 0, ox[k], 0] for k in range(8)]                             # C = 4, 4 x 8 -> 4 x 4, scalar and 16-byte path
    _run_and_compare(made("c4"), [3, 0, 1, 2, 2, 0, 3, 1], tab, (3, 4, 4), flags, f"c4 flags={flags}")


def test_time_window(made):
    tab = [[5, 0, 0, 0], [6, 0, 0, 1], [7, 0, 0, 2], [0, 0, 0, 2], [4, 0, 0, 1], [3, 0, 0, 0]]
    _run_and_compare(made("golden"), [0, 1, 2, 2, 0, 1], tab, (2, 8, 8), 3, "golden frames=2")
    _run_and_compare(made("golden"), [1, 2], [[6, 2, 4, 1], [5, 4, 0, 2]], (2, 4, 4), 3, "golden frames=2 crop 4x4")


@pytest.mark.parametrize("flags", [3, 2, 1])
def test_a_bad_table_is_clamped_not_read(made, flags):
    """Values, not a fault: rows with code 13, oy = 10^6, ox = -7 / 10^6 and t0 = -5 / 99 go straight to the entry point; the
    kernel clamps them (code & 7, or & 3 without flag bit 0; the window kept inside the source), so the whole output -- written
    into the middle of sentinel-filled buffers -- equals the launch with the clamped table, and nothing around it is touched."""
    ds, xa, ya, plain = made("golden")
    keep = 7 if flags & 1 else 3
    bad = [[13, 10 ** 6, -7, -5], [2, 1, 4, 1], [8 + 2, -1, 10 ** 6, 99], [-1, 3, 0, 2]]
    clamped = [[13 & keep, 4, 0, 0], [2, 1, 4, 1], [2, 0, 4, 2], [keep, 3, 0, 2]]
    idx, shape = [1, 0, 2, 1], (2, 4, 4)
    want = _run_and_compare((ds, xa, ya, plain), idx, clamped, shape, flags, f"clamped table, flags={flags}")
    n, SENT = len(idx), -12345.0
    big = [torch.full((n + 2, 2, c, 4, 4), SENT, device=DEV) for c in (2, 1, 1)]
    out = tuple(b[1:1 + n] for b in big)
    E._gather_augment(ds, xa, ya, torch.tensor(idx, dtype=torch.int64, device=DEV), _table(bad), n, shape, flags, out=out)
    for b, w in zip(big, want):
        assert torch.equal(b[1:1 + n], w)
        assert bool((b[0] == SENT).all()) and bool((b[-1] == SENT).all())


# ---------------------------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------------------------
def _G(seed):
    return torch.Generator().manual_seed(seed)


POSITIONS = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3]         # rows 1, 3 and 5 twice


def test_loader_reproduces_epochs_and_matches_the_plain_gather_moved(made):
    ds, xa, ya, plain = made("12")
    aug = U.Augment(hflip=True, vflip=True, transpose=True, crop=(8, 8), frames=2, crop_align=2)
    a = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, augment=aug, augment_generator=_G(5))
    b = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, augment=aug, augment_generator=_G(5))
    assert a.last_augment is None
    tables = []
    for epoch in range(2):
        ba = [tuple(t.clone() for t in batch) for batch in a]
        tab = a.last_augment
        bb = list(b)
        assert np.array_equal(tab, b.last_augment) and tab.shape == (len(POSITIONS), 4) and tab.dtype == np.int32
        assert [tuple(t[0].shape) for t in ba] == [(4, 2, 2, 8, 8), (4, 2, 2, 8, 8), (2, 2, 2, 8, 8)]
        s = 0
        for (x, y, m), other in zip(ba, bb):
            n = x.shape[0]
            want = _moved(plain, POSITIONS[s:s + n], tab[s:s + n].tolist(), (2, 8, 8))
            for got, w, o in zip((x, y, m), want, other):
                assert torch.equal(got, w) and torch.equal(got, o)
            s += n
        tables.append(tab.copy())
    assert not np.array_equal(tables[0], tables[1])                        # the generator's stream continues
    # draws are per position, not per row: the positions that name one row (3: 0 and 9, 1: 1 and 3, 5: 4 and 8) do not all agree
    assert any(not np.array_equal(t[i], t[j]) for t in tables for i, j in ((0, 9), (1, 3), (4, 8)))
    # a third loader with another seed draws another epoch
    c = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, augment=aug, augment_generator=_G(6))
    list(c)
    assert not np.array_equal(c.last_augment, tables[0])


def test_augment_none_is_the_plain_loader(made):
    ds, xa, ya, plain = made("12")
    loader = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, augment=None)
    assert loader.augment is None
    s = 0
    for x, y, m in loader:
        rows = POSITIONS[s:s + x.shape[0]]
        for got, t in zip((x, y, m), plain):
            assert torch.equal(got, t[rows])
        s += x.shape[0]
    assert s == len(POSITIONS) and loader.last_augment is None


def test_batches_write_into_static_buffers_of_the_cropped_shape(made):
    ds, xa, ya, plain = made("12")
    aug = U.Augment(hflip=True, transpose=True, crop=(8, 8), frames=2, crop_align=4)
    out = tuple(torch.empty(4, 2, c, 8, 8, device=DEV) for c in (2, 1, 1))
    loader = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, drop_last=True, augment=aug, augment_generator=_G(1))
    fresh = [tuple(t.clone() for t in batch) for batch in
             U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, drop_last=True, augment=aug, augment_generator=_G(1))]
    n = 0
    for k, (x, y, m) in enumerate(loader.batches(out=out)):
        assert x is out[0] and y is out[1] and m is out[2]
        for got, want in zip(out, fresh[k]):
            assert torch.equal(got, want)
        n += 1
    assert n == len(fresh) == 2 and not (loader.last_augment[:, 1:3] % 4).any()
    with pytest.raises(ValueError):                                        # the SOURCE shape is not the output shape
        loader.batches(out=tuple(torch.empty(4, 3, c, 12, 12, device=DEV) for c in (2, 1, 1)))
    with pytest.raises(ValueError):
        U.DeviceSequenceLoader(ds, 4, augment=U.Augment(crop=(16, 16)))   # larger than the source: refused at construction


# ---------------------------------------------------------------------------------------------
# plane_d4
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", range(8))
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 40), (2, 36, 40)])
def test_plane_d4_is_exact_and_invertible(shape, code):
    """(3, 5, 7) and (2, 33, 40) without t: scalar / 16-byte path; (2, 33, 40) with t writes rows of 33: scalar path with ragged
    tiles; (2, 36, 40) with t: 16-byte path through the LDS tile with partial tiles in both dimensions."""
    t = torch.randn(shape, generator=_G(sum(shape)), dtype=torch.float32).to(DEV)
    got = U.plane_d4(t, code)
    assert got.is_contiguous() and torch.equal(got, torch_move(t, code))
    assert torch.equal(U.plane_d4(got, inv(code)), t)
    # accumulate: one product and one add, each correctly rounded (or contracted into one fma): within 2 ulp of the f64 value
    acc0 = torch.randn(got.shape, generator=_G(1), dtype=torch.float32).to(DEV)
    acc = acc0.clone()
    assert U.plane_d4(t, code, out=acc, accumulate=True, scale=0.125) is acc
    ref = acc0.double() + 0.125 * torch_move(t, code).double()
    ulp = torch.from_numpy(np.spacing(np.abs(ref.cpu().numpy()).astype(np.float32)).astype(np.float64)).to(DEV)
    err = (acc.double() - ref).abs()
    print(f"[plane_d4] {shape} code {code}: accumulate max error {float((err / ulp).max()):.3f} ulp (bound 2)")
    assert bool((err <= 2 * ulp).all())
    with pytest.raises(ValueError):
        U.plane_d4(t, code, accumulate=True)
    with pytest.raises(ValueError):
        U.plane_d4(t, 8)


def test_plane_d4_moves_the_last_two_dims_of_a_batch():
    t = torch.randn((2, 3, 2, 8, 8), generator=_G(0)).to(DEV)
    for code in range(8):
        assert torch.equal(U.plane_d4(t, code), torch_move(t, code))
    with pytest.raises(U.UclstmError):
        U.plane_d4(t.transpose(0, 1), 1)                                   # not contiguous


# ---------------------------------------------------------------------------------------------
# predict_tta / evaluate
# ---------------------------------------------------------------------------------------------
def _ramp_model(ramp):
    """NOT equivariant: channel 0 times a fixed ramp over (H, W); returns (list of frames, None) like the model."""
    def model(x):
        y = x[:, :, :1] * ramp.to(x.dtype)
        return [y[:, t] for t in range(y.shape[1])], None
    return model


@pytest.mark.parametrize("codes", ["flips", "d4", (5, 0, 6, 3)])
def test_predict_tta_against_the_same_loop_in_f64(codes):
    B, T, S = 2, 3, 12
    # values whose products with the ramp are exact in f32, so the f32 stub and its f64 twin produce the same frames and the
    # only rounding is the accumulation
    x = (torch.randint(0, 256, (B, T, 2, S, S), generator=_G(3)).float() / 64).to(DEV)
    ramp = (1 + torch.arange(S * S, dtype=torch.float32).reshape(S, S)).to(DEV)
    cs = {"flips": (0, 1, 2, 3), "d4": tuple(range(8))}.get(codes, codes)
    stub64 = _ramp_model(ramp.double())
    ref = torch.zeros(B, T, 1, S, S, dtype=torch.float64, device=DEV)
    ymax = 0.0
    for c in cs:
        y = torch.stack(stub64(torch_move(x.double(), c))[0], dim=1)
        ymax = max(ymax, float(y.abs().max()))
        ref += torch_move(y, inv(c))
    ref /= len(cs)
    got = U.predict_tta(_ramp_model(ramp), x, codes)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, T, 1, S, S)
    err, bound = float((got.double() - ref).abs().max()), len(cs) * 2.0 ** -24 * ymax
    print(f"[predict_tta] {codes}: max error {err:.3e} (bound n * 2^-24 * max|y| = {bound:.3e})")
    assert err <= bound
    assert float((ref - torch.stack(stub64(x.double())[0], dim=1)).abs().max()) > 1.0        # the stub is not equivariant
    # an equivariant model (identity, returning a tensor): the average is the plain prediction
    ident = U.predict_tta(lambda v: (v[:, :, :1].clone(), None), x, codes)
    assert float((ident.double() - x[:, :, :1].double()).abs().max()) <= len(cs) * 2.0 ** -24 * float(x.abs().max())
    if any(c & 4 for c in cs):
        with pytest.raises(ValueError):
            U.predict_tta(_ramp_model(ramp), x[..., :8].contiguous(), codes)


def test_evaluate_with_tta_on_the_golden_model(tmp_path):
    g = load_golden("model_skip")
    p = sub(g, "p/")
    model = U.TemporalUNetDualView(1, 1, base_ch=p["inc.net.0.weight"].shape[0],
                                   lstm_layers=sum(1 for k in p if k.startswith("temporal.layers.") and k.endswith("conv.weight")),
                                   use_skip_lstm=True, use_attention="attention.conv.weight" in p).to(DEV)
    model.load_state_dict(p, strict=True)
    x = g["x"].numpy()
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "ev.npz", X=(x * 30).astype(np.float32), Y=(rng.standard_normal(x[:, :, :1].shape) * 3).astype(np.float32))
    ds = U.NPZSequenceDataset(str(tmp_path / "ev.npz"))
    loader = U.DeviceSequenceLoader(ds, x.shape[0])
    dev = torch.device(DEV)
    with U.deterministic():
        today = U.evaluate(model, loader, dev, ds, use_mask=True)
        none = U.evaluate(model, loader, dev, ds, use_mask=True, tta=None)
        flips = U.evaluate(model, loader, dev, ds, use_mask=True, tta="flips")
        rep = U.evaluate_report(model, loader, dev, ds, use_mask=True, tta="flips")
    assert torch.equal(torch.tensor(today, dtype=torch.float64), torch.tensor(none, dtype=torch.float64))
    assert len(flips) == 4 and all(math.isfinite(v) for v in flips) and flips != today
    assert len(rep) == 5 and rep[:4] == flips                               # the same launches in the same (ordered) mode
