"""GPU tests of the moving-sprite source.  uclstm_sprites_render is checked BIT FOR BIT (torch.equal, no tolerance: positions and
velocities are integers, a frame value is a byte over 255) against the output of the REFERENCE's own generator recorded in
tests/golden/sprites.npz, and, where the reference cannot go (it is square-only, 28 x 28 glyphs, two planes), against the numpy
host mirror, which tests/test_sprites_host.py pins to the same fixture.  Every output buffer is pre-filled with NaN, so an element
the kernel does not write is loud.  Then DeviceSpriteLoader, and the epoch loops / EvalReport with the loader as dataset_obj."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden_np

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import engine as E

DEV = "cuda"
V_SCALE = 5.0


@pytest.fixture(scope="module")
def golden():
    return load_golden_np("sprites")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def render(bank, table, T, C, H, W, v_scale=V_SCALE, with_raw=True, x=None):
    """One launch into NaN-filled buffers -> (x, y, mask, raw or None)."""
    n = table.shape[0]
    bank_d = torch.from_numpy(np.ascontiguousarray(bank)).to(DEV)
    table_d = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(DEV)
    x = _nan(n, T, C, H, W) if x is None else x
    y, mask = _nan(n, T, 1, H, W), _nan(n, T, 1, H, W)
    raw = _nan(n, T, 2, H, W) if with_raw else None
    got = E._render_sprites(bank_d, table_d, n, (T, C, H, W), v_scale, out=(x, y, mask), raw=raw)
    assert got[0] is x and got[1] is y and got[2] is mask
    return x, y, mask, raw


def ieee_div(vmap, v_scale):
    """``raw[:, :, 1:2] / v_scale`` as the IEEE f32 division the kernel performs, moved to the device for comparison.  Taken by
    torch on the CPU: ``tensor / python_scalar`` on a GPU tensor is NOT that division -- torch multiplies by the f32 reciprocal
    there (9 * float32(1 / 5) rounds to 1.8000001, 9 / 5 to 1.7999999), so a bit-exact check against it would ask for the
    wrong bits."""
    return (torch.as_tensor(vmap, dtype=torch.float32).cpu() / v_scale).to(DEV)


def check_against(data, x, y, mask, raw, v_scale=V_SCALE):
    """``data``: the expected [n,T,2,H,W] array (reference output or host mirror)."""
    want = torch.from_numpy(data).to(DEV)
    frame = want[:, :, 0:1]
    if raw is not None:
        assert torch.equal(raw, want)
    for c in range(x.shape[2]):
        assert torch.equal(x[:, :, c:c + 1], frame), f"channel {c}"
    assert torch.equal(y, ieee_div(data[:, :, 1:2], v_scale))
    assert torch.equal(mask, (frame > 0).float())
    assert torch.isfinite(y).all()


# ---------------------------------------------------------------------------------------------
# the kernel against the reference's own output
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_render_equals_the_reference_generator(golden, case):
    N, T, S, digits = (int(v) for v in golden["cases"][case])
    x, y, mask, raw = render(golden["bank"], golden[f"c{case}_table"], T, 2, S, S)
    check_against(golden[f"c{case}_data"], x, y, mask, raw)


# ---------------------------------------------------------------------------------------------
# ... and against the host mirror where the reference cannot go
# ---------------------------------------------------------------------------------------------
def _bank(n, gh, gw, seed):
    """Sparse random bytes: zeros inside the glyph (holes are transparent), full rows and columns at its edges."""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, 256, (n, gh, gw)).astype(np.uint8)
    b[rng.random((n, gh, gw)) < 0.4] = 0
    b[:, 0, :] |= 1
    b[:, -1, :] |= 1
    b[:, :, 0] |= 1
    b[:, :, -1] |= 1
    return b


SHAPES = {
    # name: (n_out, D, T, C, H, W, gh, gw, max_speed, with_raw)
    "40x52_noraw": (3, 2, 5, 2, 40, 52, 28, 28, 5, False),
    "36x30_scalar": (3, 3, 5, 2, 36, 30, 28, 28, 5, True),
    "glyph12x20": (4, 2, 6, 2, 40, 52, 12, 20, 7, True),
    "glyph13x7_bytes": (2, 2, 4, 2, 24, 32, 13, 7, 5, True),          # gw % 4 != 0: the byte-wise LDS fill
    "c1": (2, 2, 3, 1, 32, 32, 8, 8, 5, True),
    "c3": (2, 2, 3, 3, 32, 32, 8, 8, 5, True),
    "c3_scalar": (2, 2, 3, 3, 32, 30, 8, 8, 5, True),
    "n1_d1": (1, 1, 4, 2, 32, 32, 8, 8, 5, True),
    "n5_d8": (5, 8, 4, 2, 32, 32, 8, 8, 5, True),
    "glyph64": (2, 2, 3, 2, 72, 68, 64, 64, 9, True),                 # the largest glyph; 1224 groups: a ragged last block
    "fast": (3, 2, 8, 2, 32, 36, 28, 28, 127, True),                  # |v| far above the slack: every step bounces
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_render_equals_the_host_mirror(name):
    n, D, T, C, H, W, gh, gw, speed, with_raw = SHAPES[name]
    bank = _bank(5, gh, gw, seed=len(name))
    table = U.epoch_sprites(n, D, 5, H, W, gh, gw, speed, torch.Generator().manual_seed(7 + len(name)))
    x, y, mask, raw = render(bank, table, T, C, H, W, with_raw=with_raw)
    assert (raw is None) == (not with_raw)
    check_against(U.render_sprites_host(bank, table, T, H, W), x, y, mask, raw)


def test_hand_built_table():
    H, W, gh, gw, T = 32, 40, 28, 28, 7                                # the slack is 12 columns, 4 rows
    bank = _bank(4, gh, gw, seed=1)
    bank[3] = 0                                                        # an all-zero glyph: draws nothing, adds nothing
    table = np.array([
        [[0, 3, 1, 2, 1], [1, 3, 1, 2, 1]],                            # same start and velocity: sprite 1 on top, vmap = 2 vx
        [[3, 5, 2, 4, -3], [2, 6, 0, 0, 0]],                           # the zero glyph; velocity 0
        [[1, 12, 4, 5, 5], [2, 12, 4, -5, -5]],                        # a start at the far corner, both ways
        [[0, 0, 0, 100, -90], [1, 12, 0, -13, 127]],                   # |v| larger than the slack
    ], dtype=np.int32)
    want = U.render_sprites_host(bank, table, T, H, W)
    both = (bank[0] > 0) & (bank[1] > 0)
    assert both.any() and np.array_equal(want[0, 0, 1, 1:1 + gh, 3:3 + gw][both], np.full(both.sum(), 4.0, dtype=np.float32))
    assert np.array_equal(want[0, 0, 0, 1:1 + gh, 3:3 + gw][both], (bank[1][both] / 255.0).astype(np.float32))
    assert not want[1, :, 1].any() and np.array_equal(want[1, 0, 0], want[1, -1, 0])
    x, y, mask, raw = render(bank, table, T, 2, H, W)
    check_against(want, x, y, mask, raw)
    # another divisor: y is an IEEE division of the map, not a product with a reciprocal
    x, y, mask, raw = render(bank, table, T, 2, H, W, v_scale=3.0)
    check_against(want, x, y, mask, raw, v_scale=3.0)


def test_misaligned_output_takes_the_scalar_path_with_the_same_bits(golden):
    N, T, S, digits = (int(v) for v in golden["cases"][0])
    flat = _nan(N * T * 2 * S * S + 4)
    assert flat.data_ptr() % 16 == 0
    x_off = flat[1:1 + N * T * 2 * S * S].view(N, T, 2, S, S)
    assert x_off.data_ptr() % 16 == 4 and x_off.is_contiguous()
    x, y, mask, raw = render(golden["bank"], golden["c0_table"], T, 2, S, S, x=x_off)
    check_against(golden["c0_data"], x, y, mask, raw)
    assert torch.isnan(flat[0]) and torch.isnan(flat[-3:]).all()          # nothing outside the view was touched


def test_kernel_clamps_a_bad_table(golden):
    """The host layer refuses such a table (tests/test_sprites_host.py); handed to the library directly it is rendered as the
    table clamped into range -- never a wild access."""
    bank = golden["bank"]
    bad = np.array([[[99, 80, -3, 300, -300], [-5, -1, 70, 1, 0]]], dtype=np.int32)
    clamped = np.array([[[11, 36, 0, 127, -127], [0, 0, 36, 1, 0]]], dtype=np.int32)
    x, y, mask, raw = render(bank, bad, 4, 2, 64, 64)
    check_against(U.render_sprites_host(bank, clamped, 4, 64, 64), x, y, mask, raw)


# ---------------------------------------------------------------------------------------------
# DeviceSpriteLoader
# ---------------------------------------------------------------------------------------------
def _loader(seed=3, **kw):
    args = dict(batch_size=3, steps_per_epoch=2, T=4, H=32, W=36, num_sprites=2, generator=torch.Generator().manual_seed(seed))
    args.update(kw)
    return U.DeviceSpriteLoader(U.procedural_glyphs(6, 12), **args)


def test_loader_epochs_are_seeded_and_match_the_host_mirror():
    a, b = _loader(), _loader()
    assert len(a) == 2 and a.y_transform is None and a.y_scale == 1.0 and (a.trans_min, a.trans_max) == (-5.0, 5.0)
    ea, eb = list(a), list(b)
    assert len(ea) == 2 and np.array_equal(a.last_table, b.last_table) and a.last_table.shape == (6, 2, 5)
    for (xa, ya, ma), (xb, yb, mb) in zip(ea, eb):
        assert xa.shape == (3, 4, 2, 32, 36) and ya.shape == ma.shape == (3, 4, 1, 32, 36) and xa.dtype == torch.float32
        assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(ma, mb)
    want = torch.from_numpy(U.render_sprites_host(a.bank_host, a.last_table, 4, 32, 36)).to(DEV)
    for s, (x, y, m) in enumerate(ea):
        w = want[3 * s:3 * s + 3]
        assert torch.equal(x[:, :, 0:1], w[:, :, 0:1]) and torch.equal(x[:, :, 1:2], w[:, :, 0:1])
        assert torch.equal(y, ieee_div(w[:, :, 1:2], 5.0)) and torch.equal(m, (w[:, :, 0:1] > 0).float())
        assert torch.equal(a.denormalize(y), y * 5.0)
    first = a.last_table.copy()
    second = list(a)                                                     # the next epoch continues the stream: fresh sequences
    assert not np.array_equal(a.last_table, first) and not torch.equal(second[0][0], ea[0][0])
    assert not np.array_equal(_loader(seed=4).__iter__().__next__()[0].cpu().numpy(), ea[0][0].cpu().numpy())


def test_fixed_loader_repeats_its_epoch_and_out_buffers_are_the_callers():
    f = _loader(fixed=True)
    table = f.last_table.copy()
    e1 = [tuple(t.clone() for t in b) for b in f]
    e2 = [tuple(t.clone() for t in b) for b in f]
    assert np.array_equal(f.last_table, table)
    for b1, b2 in zip(e1, e2):
        assert all(torch.equal(u, v) for u, v in zip(b1, b2))
    assert not torch.equal(e1[0][0], e1[1][0])
    out = (_nan(3, 4, 2, 32, 36), _nan(3, 4, 1, 32, 36), _nan(3, 4, 1, 32, 36))
    n = 0
    for (x, y, m), want in zip(f.batches(out=out), e1):
        assert x is out[0] and y is out[1] and m is out[2]
        assert all(torch.equal(u, v) for u, v in zip((x, y, m), want))
        n += 1
    assert n == 2
    with pytest.raises(ValueError):
        next(f.batches(out=(out[0], out[1])))
    with pytest.raises(ValueError):
        next(f.batches(out=(out[0][:2], out[1], out[2])))


def test_loader_feeds_the_epoch_loops():
    train = U.DeviceSpriteLoader(U.procedural_glyphs(8, 12), 2, 3, T=4, H=32, W=32, generator=torch.Generator().manual_seed(0))
    val = U.DeviceSpriteLoader(U.procedural_glyphs(8, 12), 2, 2, T=4, H=32, W=32, generator=torch.Generator().manual_seed(1), fixed=True)
    torch.manual_seed(0)
    model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV)
    opt = U.FusedAdamW(model.parameters(), lr=2e-3, weight_decay=1e-4, max_grad_norm=1.0)
    tr = U.train_one_epoch(model, train, opt, torch.device(DEV), train, use_mask=True)
    ev = U.evaluate(model, val, torch.device(DEV), val, use_mask=True)
    for out in (tr, ev):
        assert len(out) == 4 and all(math.isfinite(v) for v in out), out
    assert tr[1] > 0 and ev[1] > 0                                       # an untrained model is not exact


def test_eval_report_takes_the_loader_as_dataset_obj():
    loader = _loader(fixed=True, v_scale=4.0)
    x, y, mask = next(iter(loader))
    y_pred = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    rep = U.EvalReport(loader)
    rep.add(y, y_pred, mask, use_mask=False)
    got = rep.result()
    want = float(((y_pred.double() - y.double()).abs() * 4.0).mean())
    assert got["n"] == y.numel() and abs(got["mae"] - want) <= 1e-6 * want, (got["mae"], want)
