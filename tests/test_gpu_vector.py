"""GPU tests of the vector-target data path.  uclstm_dataset_gather_vec BIT FOR BIT against (a) uclstm_dataset_gather_transform per
channel, (b) its own plain output on raw data moved on the host with torch.flip / transpose / channel permutation / negation and
(c) uclstm_dataset_gather_augment at Cy = 1; clamping of bad tables; the physics of a gradient field through the kernel; then
DeviceSequenceLoader over a VectorNPZDataset, uclstm_plane_d4_vec and predict_tta(dataset=...).  Shapes are those of
tests/test_gpu_augment.py: 40 x 40 (two LDS tiles per side, the second partial, 16-byte path), 5 x 7 (scalar path, non-square),
12 x 12, C in {2, 3} (compile-time / run-time channel loop)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vector_cases as VC
from vector_cases import torch_move, inv

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import engine as E
    from unet_convlstm_amd import ops

DEV = "cuda"
TRANSFORMS = ["asinh", "signed_log", None]
# case -> (N, T, C, Cy, H, W, axes)
SHAPES = {"40": (3, 2, 2, 3, 40, 40, VC.AXES_UVW), "5x7": (5, 1, 2, 2, 5, 7, ("-w", "+h")), "c3": (4, 3, 3, 4, 4, 8, ("+h", None, "-w", None)),
          "12": (10, 3, 2, 3, 12, 12, VC.AXES_UVW), "8": (3, 4, 2, 2, 8, 8, ("+w", "+h")), "one": (3, 4, 2, 1, 8, 8, (None,)), "one_neg": (3, 4, 2, 1, 8, 8, ("-w",))}
_cache = {}


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(case, transform, clip) -> (dataset, x_all, y_all on the device, the PLAIN vector gather of every row in order); built once,
    never changed."""
    root = tmp_path_factory.mktemp("vector")

    def get(case, transform="asinh", clip=True):
        key = (case, transform, clip)
        if key not in _cache:
            N, T, Cc, Cy, H, W, axes = SHAPES[case]
            path = root / f"{case}.npz"
            if not path.exists():
                VC.write_npz(path, N, T, Cc, Cy, H, W, seed=len(case) + 7)
            ds = U.VectorNPZDataset(str(path), axes, tie_horizontal=(case == "12"), y_transform=transform, clip_outliers=clip,
                                    lower_percentile=1.0, upper_percentile=99.0)
            xa, ya = torch.from_numpy(ds.X).to(DEV), torch.from_numpy(ds.Y).to(DEV)
            _cache[key] = (ds, xa, ya, E._gather_vec(ds, xa, ya, None, None, len(ds), (T, H, W), 2))
        return _cache[key]
    return get


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(-1, 4)


def _idx(idx):
    return torch.tensor(idx, dtype=torch.int64, device=DEV)


def _moved_raw(ds, xa, ya, idx, tab, shape, cmap=None):
    """The raw data of rows ``idx`` moved on the host side of the check: window, flip / transpose, channel map with negation
    (``cmap(code)``; None: the dataset's ``channel_map``)."""
    cmap = cmap or ds.channel_map
    To, Ho, Wo = shape
    xs, ys = [], []
    for row, (code, oy, ox, t0) in zip(idx, tab):
        Hc, Wc = (Wo, Ho) if code & 4 else (Ho, Wo)
        xs.append(torch_move(xa[row, t0:t0 + To, :, oy:oy + Hc, ox:ox + Wc], code))
        ys.append(VC.apply_map(ya[row, t0:t0 + To, :, oy:oy + Hc, ox:ox + Wc], code, cmap(code)))
    return torch.stack(xs).contiguous(), torch.stack(ys).contiguous()


def _run_and_compare(made_case, idx, tab, shape, flags, what, cmap=None):
    """Equality (b): the augmented batch equals the PLAIN vector gather (aug = NULL) of the raw data moved with torch."""
    ds, xa, ya, _ = made_case
    got = E._gather_vec(ds, xa, ya, _idx(idx), _table(tab), len(idx), shape, flags)
    xr, yr = _moved_raw(ds, xa, ya, idx, tab, shape, cmap)
    want = E._gather_vec(ds, xr, yr, None, None, len(idx), shape, 2)
    for g, w, name, ch in zip(got, want, ("x", "y", "mask"), (xa.shape[2], ds.Cy, 1)):
        assert tuple(g.shape) == (len(idx), shape[0], ch, shape[1], shape[2]) and g.is_contiguous(), (what, name)
        assert torch.equal(g, w), f"{what}: {name} differs in {int((g != w).sum())} of {g.numel()} elements"
    return got


# ---------------------------------------------------------------------------------------------
# (a) without aug: channel c is uclstm_dataset_gather_transform on channel c with its constants
# ---------------------------------------------------------------------------------------------
class _Scalar:
    """The scalar view of one channel's constants, as _gather_transform reads them."""

    def __init__(self, ds, c):
        self.y_transform, self.norm_const, self.clip_outliers = ds.y_transform, ds.norm_const, ds.clip_outliers
        self.min_vel, self.max_vel, self.y_scale = ds.min_vel[c], ds.max_vel[c], ds.y_scale[c]
        self.trans_min, self.trans_max = ds.trans_min[c], ds.trans_max[c]


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("transform", TRANSFORMS, ids=str)
@pytest.mark.parametrize("case", ["40", "5x7", "c3", "one_neg"])
def test_plain_gather_equals_the_scalar_kernel_per_channel(made, case, transform, clip):
    ds, xa, ya, plain = made(case, transform, clip)
    idx = [len(ds) - 1, 0, 1, 1]
    x, y, m = E._gather_vec(ds, xa, ya, _idx(idx), None, len(idx), xa.shape[1:2] + xa.shape[3:], 2)
    assert tuple(y.shape) == (len(idx), xa.shape[1], ds.Cy) + tuple(xa.shape[3:])
    for c in range(ds.Cy):
        sx, sy, sm = E._gather_transform(_Scalar(ds, c), xa, ya[:, :, c:c + 1].contiguous(), _idx(idx), len(idx))
        assert torch.equal(y[:, :, c:c + 1], sy), f"{case} {transform} clip={clip}: channel {c} differs in {int((y[:, :, c:c + 1] != sy).sum())}"
        assert torch.equal(x, sx) and torch.equal(m, sm)
    for t, p in zip((x, y, m), plain):
        assert torch.equal(t, p[idx])
    if transform == "asinh" and clip:                                      # ... and against the host dataset, not a kernel alone
        hx, hy, hm = ds[idx[0]]
        torch.testing.assert_close(y[0].cpu(), hy, rtol=1e-5, atol=2e-6)
        torch.testing.assert_close(x[0].cpu(), hx, rtol=1e-6, atol=1e-7)
        assert torch.equal(m[0].cpu(), hm)
    # device_transform takes the same kernel in identity order
    dx, dy, dm = U.device_transform(ds, xa[:2], ya[:2])
    assert torch.equal(dx, plain[0][:2]) and torch.equal(dy, plain[1][:2]) and torch.equal(dm, plain[2][:2])


# ---------------------------------------------------------------------------------------------
# (b) with aug: the plain gather of the raw data moved on the host
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("transform", TRANSFORMS, ids=str)
def test_full_frame_all_codes_16_byte_path(made, transform, clip):
    tab = [[k, 0, 0, 0] for k in range(8)]
    x, y, m = _run_and_compare(made("8", transform, clip), [2, 0, 2, 1, 0, 2, 1, 1], tab, (4, 8, 8), 3, f"8 {transform} clip={clip}")
    assert not torch.equal(y[0], y[2])                                     # the same row under code 0 and code 2


@pytest.mark.parametrize("crop,oy,ox,flags", [(36, 1, 3, 1), (36, 4, 4, 3), (33, 7, 0, 3), (33, 7, 0, 1)])
def test_partial_tiles_in_both_dimensions(made, crop, oy, ox, flags):
    tab = [[k, oy, ox, 0] for k in range(8)]
    _run_and_compare(made("40"), [0, 1, 2, 0, 1, 2, 0, 1], tab, (2, crop, crop), flags, f"40 crop {crop} at ({oy}, {ox})")


def test_non_square_frames_take_the_codes_without_t(made):
    case = made("5x7")
    ds, xa, ya, _ = case
    _run_and_compare(case, [4, 0, 3, 3, 1], [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0], [3, 0, 0, 0], [3, 0, 0, 0]], (1, 5, 7), 0, "5x7")
    _run_and_compare(case, [2, 1, 0, 4], [[k, 1, 2, 0] for k in range(4)], (1, 3, 4), 0, "5x7 crop 3x4")
    with pytest.raises(U.UclstmError):                                     # a table that may hold t needs Ho == Wo
        E._gather_vec(ds, xa, ya, None, _table([[4, 0, 0, 0]]), 1, (1, 5, 7), 1)


@pytest.mark.parametrize("ox,flags", [([0, 4, 2, 4, 0, 1, 3, 4], 1), ([0, 4, 4, 0, 4, 0, 0, 4], 3)])
def test_run_time_channel_loop_and_four_target_channels(made, ox, flags):
    tab = [[k, 0, ox[k], 0] for k in range(8)]                             # C = 3, Cy = 4, 4 x 8 -> 4 x 4, scalar and 16-byte path
    _run_and_compare(made("c3"), [3, 0, 1, 2, 2, 0, 3, 1], tab, (3, 4, 4), flags, f"c3 flags={flags}")


def test_time_window(made):
    tab = [[5, 0, 0, 0], [6, 0, 0, 1], [7, 0, 0, 2], [0, 0, 0, 2], [4, 0, 0, 1], [3, 0, 0, 0]]
    _run_and_compare(made("8"), [0, 1, 2, 2, 0, 1], tab, (2, 8, 8), 3, "8 frames=2")
    _run_and_compare(made("8"), [1, 2], [[6, 2, 4, 1], [5, 4, 0, 2]], (2, 4, 4), 3, "8 frames=2 crop 4x4")


# ---------------------------------------------------------------------------------------------
# (c) Cy = 1, axes (None,): the scalar augmenting kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", TRANSFORMS, ids=str)
@pytest.mark.parametrize("shape,flags,oyx", [((4, 8, 8), 3, (0, 0)), ((2, 4, 4), 3, (4, 4)), ((3, 5, 5), 1, (1, 3))])
def test_one_scalar_channel_equals_the_scalar_augment_kernel(made, transform, shape, flags, oyx):
    ds, xa, ya, _ = made("one", transform, True)
    idx = [2, 0, 2, 1, 0, 2, 1, 1]
    tab = _table([[k, oyx[0], oyx[1], k % (5 - shape[0])] for k in range(8)])
    got = E._gather_vec(ds, xa, ya, _idx(idx), tab, 8, shape, flags)
    want = E._gather_augment(_Scalar(ds, 0), xa, ya, _idx(idx), tab, 8, shape, flags)
    for g, w, name in zip(got, want, ("x", "y", "mask")):
        assert torch.equal(g, w), f"{transform} {shape}: {name} differs in {int((g != w).sum())} of {g.numel()} elements"


# ... and one channel whose map negates: what only the instantiation for Cy = 1 can get wrong
@pytest.mark.parametrize("transform", TRANSFORMS, ids=str)
@pytest.mark.parametrize("shape,flags,oyx", [((4, 8, 8), 3, (0, 0)), ((3, 5, 5), 1, (1, 3))])
def test_one_channel_that_negates_under_mirrors(made, transform, shape, flags, oyx):
    """Cy = 1, axes ("-w",): the channel changes sign under h.  With a single horizontal channel ``channel_map`` refuses the codes
    with t and ``chan_map_table`` holds identity rows for them, so the reference reads the rows the kernel is given."""
    case = made("one_neg", transform, True)
    ds = case[0]
    table = ds.chan_map_table().view(np.uint8)

    def cmap(code):
        return [(int(table[code, 0]) & 7, bool(table[code, 0] & 0x80))]
    assert all(cmap(k) == ds.channel_map(k) for k in range(4))
    assert [cmap(k)[0][1] for k in range(8)] == [False, True, False, True, False, False, False, False]      # not vacuous: codes 1, 3 negate
    tab = [[k, oyx[0], oyx[1], k % (5 - shape[0])] for k in range(8)]
    _, y, _ = _run_and_compare(case, [2, 0, 2, 1, 0, 2, 1, 1], tab, shape, flags, f"one_neg {transform} {shape}", cmap)
    assert not torch.equal(y[0], y[2])                                     # the same row and window under code 0 and code 2


def test_both_instantiations_in_one_process_agree_on_x_and_mask(made):
    """One launch at Cy = 2 and one at Cy = 1 over the same x_all, both without a table: x and mask do not know about Cy, and target
    channel 0 (identity map, the same constants) does not either."""
    ds, xa, ya, _ = made("8")
    N, T, Cc, H, W = xa.shape
    consts = ds.target_consts()
    outs = []
    for Cy, y_all in ((2, ya), (1, ya[:, :, :1].contiguous())):
        out = tuple(torch.empty(N, T, c, H, W, device=DEV) for c in (Cc, Cy, 1))
        L.check(L.lib.uclstm_dataset_gather_vec(ops._p(xa), ops._p(y_all), None, None, N, N, T, T, Cc, Cy, H, W, H, W, 2, None,
                                                ops._p(out[0]), ops._p(out[1]), ops._p(out[2]), 1, float(ds.norm_const), 1, consts,
                                                ops._stream()), "gather_vec")
        outs.append(out)
    (x2, y2, m2), (x1, y1, m1) = outs
    assert torch.equal(x2, x1) and torch.equal(m2, m1)
    assert torch.equal(y2[:, :, :1], y1)


# ---------------------------------------------------------------------------------------------
# clamping
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [3, 2, 1])
def test_bad_tables_are_clamped_not_read(made, flags):
    """Values, not a fault: table rows with code 13, oy = 10^6, ox = -7 / 10^6, t0 = -5 / 99 and a channel map whose source channels
    are 5, 6 and 7 go straight to the entry point.  The kernel clamps them (code & 7, or & 3 without flag bit 0; the window kept
    inside the source; the source channel into [0, Cy)), so the output -- written into the middle of sentinel-filled buffers --
    equals the launch with the clamped tables, and nothing around it is touched."""
    ds, xa, ya, _ = made("8")
    N, T, Cc, H, W = xa.shape
    keep = 7 if flags & 1 else 3
    bad = [[13, 10 ** 6, -7, -5], [2, 1, 4, 1], [8 + 2, -1, 10 ** 6, 99], [-1, 3, 0, 2]]
    clamped = [[13 & keep, 4, 0, 0], [2, 1, 4, 1], [2, 0, 4, 2], [keep, 3, 0, 2]]
    idx, shape, n, SENT = [1, 0, 2, 1], (2, 4, 4), 4, -12345.0
    bad_map = np.array([[5 | 0x80, 6]] * 4 + [[7, 0x80 | 0x40 | 3]] * 4, dtype=np.uint8).view(np.int8)      # sources 5, 6, 7, 3 -> 1
    clamped_map = np.array([[1 | 0x80, 1]] * 4 + [[1, 0x80 | 1]] * 4, dtype=np.uint8).view(np.int8)
    consts = ds.target_consts()

    def launch(tab, cmap, rows, out):
        rows, tab = _idx(rows), _table(tab)
        L.check(L.lib.uclstm_dataset_gather_vec(ops._p(xa), ops._p(ya), ops._p(rows), ops._p(tab), N, n, T, shape[0], Cc, 2,
                                                H, W, shape[1], shape[2], flags, cmap.ctypes.data, ops._p(out[0]), ops._p(out[1]),
                                                ops._p(out[2]), 1, float(ds.norm_const), 1, consts, ops._stream()), "gather_vec")
        torch.cuda.synchronize()
    want = tuple(torch.empty(n, 2, c, 4, 4, device=DEV) for c in (2, 2, 1))
    launch(clamped, clamped_map, idx, want)
    # what the clamped tables mean, with torch: both output channels read source channel 1, negated as the map says
    code_neg = {k: ((True, False) if k < 4 else (False, True)) for k in range(8)}
    xr = torch.stack([torch_move(xa[r, t0:t0 + 2, :, oy:oy + 4, ox:ox + 4], k) for r, (k, oy, ox, t0) in zip(idx, clamped)]).contiguous()
    yr = torch.stack([torch.stack([(-1.0 if code_neg[k][c] else 1.0) * torch_move(ya[r, t0:t0 + 2, 1, oy:oy + 4, ox:ox + 4], k)
                                   for c in range(2)], dim=1) for r, (k, oy, ox, t0) in zip(idx, clamped)]).contiguous()
    ref = E._gather_vec(ds, xr, yr, None, None, n, shape, 2)
    for w, r in zip(want, ref):
        assert torch.equal(w, r)
    big = [torch.full((n + 2, 2, c, 4, 4), SENT, device=DEV) for c in (2, 2, 1)]
    launch(bad, bad_map, [1, -9, 2 + 10 ** 9, 1], tuple(b[1:1 + n] for b in big))          # rows clamp to 0 and N - 1 = 2
    for b, w in zip(big, want):
        assert torch.equal(b[1:1 + n], w)
        assert bool((b[0] == SENT).all()) and bool((b[-1] == SENT).all())


# ---------------------------------------------------------------------------------------------
# the physics through the kernel: exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes", [VC.AXES_UVW, ("-h", None, "-w"), ("+w", "+h")], ids=str)
@pytest.mark.parametrize("S", [12, 40])
def test_the_gradient_field_through_the_kernel_is_exact(tmp_path, axes, S):
    """Raw targets = the integer gradient field of vector_cases.potential_field; transform none, clip off, bounds -K .. K with
    K = 2^23 > |v|: v + K is an integer below 2^24 and y = 2 (v + K) / 2K - 1 = v / K exactly in f32, contracted or not.  All eight
    codes in one launch must give the field of the MOVED potential."""
    K = float(2 ** 23)
    field = VC.potential_field(axes, S, 0).astype(np.float32)
    assert float(np.abs(field).max()) < K
    rng = np.random.default_rng(S)
    np.savez(tmp_path / "phi.npz", X=(rng.random((1, 1, 2, S, S)) * 30).astype(np.float32), Y=field[None, None])
    ds = U.VectorNPZDataset(str(tmp_path / "phi.npz"), axes, y_transform=None, clip_outliers=False, min_y=-K, max_y=K)
    xa, ya = torch.from_numpy(ds.X).to(DEV), torch.from_numpy(ds.Y).to(DEV)
    _, y, _ = E._gather_vec(ds, xa, ya, _idx([0] * 8), _table([[k, 0, 0, 0] for k in range(8)]), 8, (1, S, S), 3)
    for code in range(8):
        want = torch.from_numpy(VC.potential_field(axes, S, code).astype(np.float64) / K).float()
        got = y[code, 0].cpu()
        assert torch.equal(got, want), f"axes {axes} S={S} code {code}: {int((got != want).sum())} values differ"


# ---------------------------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------------------------
def _G(seed):
    return torch.Generator().manual_seed(seed)


POSITIONS = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3]


def test_loader_reproduces_epochs_and_matches_the_moved_raw_data(made):
    case = made("12")
    ds, xa, ya, plain = case
    aug = U.Augment(hflip=True, vflip=True, transpose=True, crop=(8, 8), frames=2, crop_align=2)
    a = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, augment=aug, augment_generator=_G(5))
    b = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, augment=aug, augment_generator=_G(5))
    tables = []
    for epoch in range(2):
        ba = [tuple(t.clone() for t in batch) for batch in a]
        tab = a.last_augment
        bb = list(b)
        assert np.array_equal(tab, b.last_augment) and tab.shape == (len(POSITIONS), 4)
        assert [tuple(t[1].shape) for t in ba] == [(4, 2, 3, 8, 8), (4, 2, 3, 8, 8), (2, 2, 3, 8, 8)]
        assert [tuple(t[2].shape) for t in ba] == [(4, 2, 1, 8, 8), (4, 2, 1, 8, 8), (2, 2, 1, 8, 8)]
        s = 0
        for (x, y, m), other in zip(ba, bb):
            n = x.shape[0]
            xr, yr = _moved_raw(ds, xa, ya, POSITIONS[s:s + n], tab[s:s + n].tolist(), (2, 8, 8))
            want = E._gather_vec(ds, xr, yr, None, None, n, (2, 8, 8), 2)
            for got, w, o in zip((x, y, m), want, other):
                assert torch.equal(got, w) and torch.equal(got, o)
            s += n
        tables.append(tab.copy())
    assert not np.array_equal(tables[0], tables[1]) and bool((np.concatenate(tables)[:, 0] & 4).any())      # swaps took place
    # augment=None: the same kernel without a table
    s = 0
    for x, y, m in U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS):
        rows = POSITIONS[s:s + x.shape[0]]
        for got, t in zip((x, y, m), plain):
            assert torch.equal(got, t[rows])
        s += x.shape[0]
    assert s == len(POSITIONS)
    # through Subsets, as random_split returns them
    sub = torch.utils.data.Subset(ds, [7, 2, 9])
    (x, y, m), = list(U.DeviceSequenceLoader(sub, 3))
    assert torch.equal(y, plain[1][[7, 2, 9]])


def test_batches_write_into_static_buffers_with_the_target_channels(made):
    ds, xa, ya, plain = made("12")
    aug = U.Augment(hflip=True, transpose=True, crop=(8, 8), frames=2, crop_align=4)
    out = tuple(torch.empty(4, 2, c, 8, 8, device=DEV) for c in (2, 3, 1))
    loader = U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, drop_last=True, augment=aug, augment_generator=_G(1))
    fresh = [tuple(t.clone() for t in batch) for batch in
             U.DeviceSequenceLoader(ds, 4, sampler=POSITIONS, drop_last=True, augment=aug, augment_generator=_G(1))]
    n = 0
    for k, (x, y, m) in enumerate(loader.batches(out=out)):
        assert x is out[0] and y is out[1] and m is out[2]
        for got, want in zip(out, fresh[k]):
            assert torch.equal(got, want)
        n += 1
    assert n == len(fresh) == 2
    with pytest.raises(ValueError):                                        # the scalar shape of y is not this loader's
        loader.batches(out=tuple(torch.empty(4, 2, c, 8, 8, device=DEV) for c in (2, 1, 1)))


def test_a_transpose_with_one_horizontal_channel_is_refused_at_construction(tmp_path):
    VC.write_npz(tmp_path / "one_h.npz", 3, 2, 2, 2, 8, 8, seed=1)
    ds = U.VectorNPZDataset(str(tmp_path / "one_h.npz"), ("+w", None))
    with pytest.raises(ValueError):
        U.DeviceSequenceLoader(ds, 2, augment=U.Augment(transpose=True))
    x, y, m = next(iter(U.DeviceSequenceLoader(ds, 2, augment=U.Augment(hflip=True, vflip=True), augment_generator=_G(0))))
    assert tuple(y.shape) == (2, 2, 2, 8, 8)


def test_a_scalar_dataset_still_launches_only_the_old_entry_points(tmp_path, monkeypatch):
    rng = np.random.default_rng(2)
    np.savez(tmp_path / "s.npz", X=(rng.random((6, 2, 2, 8, 8)) * 30).astype(np.float32), Y=rng.normal(0, 3, (6, 2, 1, 8, 8)).astype(np.float32))
    ds = U.NPZSequenceDataset(str(tmp_path / "s.npz"))
    calls = []
    for name in ("uclstm_dataset_gather_transform", "uclstm_dataset_gather_augment", "uclstm_dataset_gather_vec", "uclstm_plane_d4",
                 "uclstm_plane_d4_vec", "uclstm_metric_sums_vec", "uclstm_loss_spec_fwd_bc", "uclstm_loss_spec_bwd_bc"):
        fn = getattr(L.lib, name)
        monkeypatch.setattr(L.lib, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(fn, name))
    list(U.DeviceSequenceLoader(ds, 3))
    list(U.DeviceSequenceLoader(ds, 3, augment=U.Augment(hflip=True, transpose=True), augment_generator=_G(0)))
    x = torch.rand(1, 2, 2, 8, 8, device=DEV)
    U.predict_tta(lambda v: (v[:, :, :1].clone(), None), x, "d4")
    y = torch.rand(1, 2, 1, 8, 8, device=DEV)
    U.compute_loss(y.clone().requires_grad_(True), y, (y > 0.5).float(), True).backward()
    assert set(calls) == {"uclstm_dataset_gather_transform", "uclstm_dataset_gather_augment", "uclstm_plane_d4"}, calls
    assert calls.count("uclstm_dataset_gather_transform") == 2 and calls.count("uclstm_dataset_gather_augment") == 2
    assert calls.count("uclstm_plane_d4") == 16


# ---------------------------------------------------------------------------------------------
# plane_d4_vec
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", range(8))
@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 2, 33, 40), (2, 4, 36, 40), (3, 1, 5, 7), (2, 1, 36, 40)])
def test_plane_d4_vec_equals_signed_plane_d4_per_channel(shape, code):
    t = torch.randn(shape, generator=_G(sum(shape)), dtype=torch.float32).to(DEV)
    Cy = shape[1]
    affine = [((c + 1) % Cy, -1.0 if c % 2 == 0 else 1.0, 0.0) for c in range(Cy)]
    got = U.plane_d4_vec(t, code, affine)
    assert got.is_contiguous() and tuple(got.shape) == tuple(torch_move(t, code).shape)
    for c, (src, sign, _) in enumerate(affine):
        want = U.plane_d4(t[:, src].contiguous(), code)
        assert torch.equal(got[:, c], -want if sign < 0 else want), (shape, code, c)
    # with offsets, a scale and an accumulator, against f64: the sum v + offset, the product with scale and the final add are
    # three f32 roundings, of at most 2^-24 (V + O), 2^-24 |scale| (V + O) and 2^-24 (D + |scale| (V + O)); for |scale| >= 1 that is
    # within 3 * 2^-24 * |scale| * (V + O + D)
    offs = [0.75, -1.5, 0.3, 2.0][:Cy]
    affine = [(src, sign, off) for (src, sign, _), off in zip(affine, offs)]
    acc0 = torch.randn(got.shape, generator=_G(1), dtype=torch.float32).to(DEV)
    for scale, accumulate in ((1.0, True), (-2.5, True), (1.5, False)):
        acc = acc0.clone()
        assert U.plane_d4_vec(t, code, affine, out=acc, accumulate=accumulate, scale=scale) is acc
        ref = VC.apply_affine(t.double(), code, affine) * scale + (acc0.double() if accumulate else 0.0)
        bound = 3 * 2.0 ** -24 * abs(scale) * (float(t.abs().max()) + max(abs(o) for o in offs) + float(acc0.abs().max()) * accumulate)
        err = float((acc.double() - ref).abs().max())
        print(f"[plane_d4_vec] {shape} code {code} scale {scale} accumulate {accumulate}: max error {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    with pytest.raises(ValueError):
        U.plane_d4_vec(t, code, affine, accumulate=True)
    with pytest.raises(ValueError):
        U.plane_d4_vec(t, 8, affine)
    with pytest.raises(ValueError):
        U.plane_d4_vec(t, code, affine[:-1] + [(Cy, 1.0, 0.0)])


def test_plane_d4_keeps_the_sign_of_a_zero():
    """uclstm_plane_d4 runs the kernel of uclstm_plane_d4_vec with the offset -0.f: v + -0.f is v for v = -0.f too (+0.f would not be)."""
    t = torch.tensor([0.0, -0.0, 1.5, -2.0] * 10, device=DEV).reshape(1, 5, 8)
    for code in (0, 3, 5):
        got = U.plane_d4(t, code)
        assert torch.equal(got.view(torch.int32), torch_move(t, code).contiguous().view(torch.int32)), code


def test_plane_d4_vec_clamps_the_source_channel():
    t = torch.randn((2, 3, 8, 8), generator=_G(9)).to(DEV)
    big = torch.full((4, 3, 8, 8), -7.0, device=DEV)
    cmap = (C.c_int8 * 3)(7, 6 - 128, 1)                                    # sources 7, 6 (negated), 1 -> 2, -2, 1
    L.check(L.lib.uclstm_plane_d4_vec(ops._p(t), ops._p(big[1:3]), 2, 3, 8, 8, 5, C.addressof(cmap), None, 0, 1.0, ops._stream()), "plane_d4_vec")
    m = torch_move(t, 5)
    assert torch.equal(big[1:3], torch.stack((m[:, 2], -m[:, 2], m[:, 1]), dim=1))
    assert bool((big[0] == -7.0).all()) and bool((big[3] == -7.0).all())


# ---------------------------------------------------------------------------------------------
# predict_tta(dataset=...)
# ---------------------------------------------------------------------------------------------
def _ramp_model(ramp, gains):
    """NOT equivariant: channel 0 times a fixed ramp over (H, W), times one gain per output channel."""
    def model(x):
        y = x[:, :, :1] * ramp.to(x.dtype) * gains.to(x.dtype).view(1, 1, -1, 1, 1)
        return [y[:, t] for t in range(y.shape[1])], None
    return model


@pytest.mark.parametrize("codes", ["flips", "d4", (5, 0, 6, 3)])
def test_predict_tta_with_a_vector_dataset_against_the_same_loop_in_f64(made, codes):
    ds = made("12")[0]                                                     # tie_horizontal=True, axes (+w, -h, None)
    B, T, S = 2, 3, 12
    x = (torch.randint(0, 256, (B, T, 2, S, S), generator=_G(3)).float() / 64).to(DEV)
    ramp = (1 + torch.arange(S * S, dtype=torch.float32).reshape(S, S)).to(DEV)
    gains = torch.tensor([1.0, -0.5, 0.25], device=DEV)                    # products stay exact in f32
    cs = {"flips": (0, 1, 2, 3), "d4": tuple(range(8))}.get(codes, codes)
    stub64 = _ramp_model(ramp.double(), gains.double())
    ref = torch.zeros(B, T, 3, S, S, dtype=torch.float64, device=DEV)
    ymax, omax = 0.0, 0.0
    for c in cs:
        y = torch.stack(stub64(torch_move(x.double(), c))[0], dim=1)
        aff = ds.tta_affine(inv(c))
        ymax, omax = max(ymax, float(y.abs().max())), max(omax, max(abs(o) for _, _, o in aff))
        ref += VC.apply_affine(y, inv(c), aff)
    ref /= len(cs)
    got = U.predict_tta(_ramp_model(ramp, gains), x, codes, dataset=ds)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, T, 3, S, S)
    # the scalar test's form, n * 2^-24 * max|y| for the n accumulating adds, with M = max|y| + max|offset| as the magnitude; the
    # sum y + offset and the product with 1 / n round once more each, by at most 2^-24 M / n per code: (n + 2) * 2^-24 * M
    err, bound = float((got.double() - ref).abs().max()), (len(cs) + 2) * 2.0 ** -24 * (ymax + omax)
    print(f"[predict_tta vector] {codes}: max error {err:.3e} (bound (n + 2) * 2^-24 * (max|y| + max|offset|) = {bound:.3e})")
    assert err <= bound
    plain = U.predict_tta(_ramp_model(ramp, gains), x, codes)
    assert float((plain.double() - ref).abs().max()) > 1.0                 # without the dataset the channels do not turn
