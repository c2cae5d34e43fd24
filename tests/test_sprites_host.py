"""CPU-only tests of the moving-sprite source: the numpy host mirror against fixtures written by the REFERENCE's own generator
(tests/golden/make_sprites_golden.py: bit for bit, positions and velocities are integers and a frame value is a byte over 255),
the epoch table, the table check, the glyph banks, and the C ABI of uclstm_sprites_render (symbol, argument contract -- nothing
is launched)."""
import ctypes as C
import gzip
import hashlib
import re

import numpy as np
import pytest
import torch

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from conftest import load_golden_np

RENDER = "uclstm_sprites_render"
PROCEDURAL_SHA256 = "dcdab138a4ecf66fe395bb75d99384220c9c2b8c5abfb15da79965616373ef81"          # procedural_glyphs(12, 28, seed=0)


def _G(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def golden():
    return load_golden_np("sprites")


# ---------------------------------------------------------------------------------------------
# render_sprites_host
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_host_mirror_equals_the_reference_generator(golden, case):
    N, T, S, digits = (int(v) for v in golden["cases"][case])
    table, data = golden[f"c{case}_table"], golden[f"c{case}_data"]
    assert table.shape == (N, digits, 5) and data.shape == (N, T, 2, S, S) and data.dtype == np.float32
    got = U.render_sprites_host(golden["bank"], table, T, S, S)
    assert got.dtype == np.float32 and np.array_equal(got, data)


def test_fixture_covers_what_it_is_meant_to(golden):
    cases = [tuple(int(v) for v in c) for c in golden["cases"]]
    assert cases == [(6, 12, 64, 2), (4, 40, 64, 3), (5, 9, 28, 2), (5, 9, 31, 4), (3, 1, 64, 1)]
    assert golden["bank"].shape == (12, 28, 28) and golden["bank"].dtype == np.uint8
    assert np.abs(golden["c3_data"][:, :, 1]).max() > 5            # overlapping sprites: sums above a single speed
    # the frame equals the glyph: every sprite sits at (0, 0) in every frame, so all frames of a sequence are equal
    assert np.array_equal(golden["c2_data"][:, 0, 0], golden["c2_data"][:, -1, 0])


def test_host_mirror_non_square_and_overwrite_order():
    bank = np.zeros((2, 2, 3), dtype=np.uint8)
    bank[0] = [[255, 0, 51], [0, 102, 0]]
    bank[1] = [[0, 204, 0], [153, 0, 0]]
    table = np.array([[[0, 1, 1, 2, -1], [1, 1, 1, 2, -1]]], dtype=np.int32)      # same start, same velocity
    out = U.render_sprites_host(bank, table, 3, 4, 6)
    assert out.shape == (1, 3, 2, 4, 6)
    want = np.zeros((4, 6), dtype=np.float32)
    want[1, 1:4] = [1.0, 0.8, 0.2]                                                  # sprite 1 lies on top where it is non-zero
    want[2, 1:3] = [0.6, 0.4]
    assert np.array_equal(out[0, 0, 0], want)                                       # 204 / 255 = 0.8 ... are exact quotients
    assert np.array_equal(out[0, 0, 1], np.where(want > 0, 2.0, 0.0).astype(np.float32))      # no pixel is covered twice here
    # t = 1: x 1 -> 3 (the slack is 3), y 1 -> 0; t = 2: x 5 > 3 bounces to 3 with vx = -2, y -1 bounces to 0 with vy = +1
    assert np.array_equal(np.argwhere(out[0, 1, 0] > 0), np.argwhere(np.pad(want[1:3, 1:4], ((0, 2), (3, 0))) > 0))
    assert np.array_equal(out[0, 2, 0], out[0, 1, 0])
    assert set(np.unique(out[0, 1, 1]).tolist()) == {0.0, 2.0}                     # drawn before the step that bounces
    assert set(np.unique(out[0, 2, 1]).tolist()) == {0.0, -2.0}                    # the CURRENT vx: the flipped sign
    out4 = U.render_sprites_host(bank, table, 4, 4, 6)
    assert np.array_equal(out4[0, :3], out[0]) and np.array_equal(out4[0, 3, 0], out[0, 0, 0])      # back at (1, 1), moving left
    assert np.array_equal(out4[0, 3, 1], -out[0, 0, 1])
    # both sprites cover a common pixel: the map adds both speeds, the frame keeps the later sprite
    both = np.full((2, 1, 1), 255, dtype=np.uint8)
    both[1] = 51
    o = U.render_sprites_host(both, np.array([[[0, 2, 1, 3, 0], [1, 2, 1, -1, 0]]], dtype=np.int32), 1, 3, 5)
    assert o[0, 0, 0, 1, 2] == np.float32(0.2) and o[0, 0, 1, 1, 2] == 2.0 and np.count_nonzero(o) == 2


# ---------------------------------------------------------------------------------------------
# epoch_sprites / check_sprite_table
# ---------------------------------------------------------------------------------------------
def test_a_seed_reproduces_the_table_and_the_stream_continues():
    args = (40, 3, 12, 64, 48, 28, 20, 5)
    a, b, c = U.epoch_sprites(*args, _G(3)), U.epoch_sprites(*args, _G(3)), U.epoch_sprites(*args, _G(4))
    assert a.dtype == np.int32 and a.shape == (40, 3, 5) and np.array_equal(a, b) and not np.array_equal(a, c)
    g = _G(3)
    first, second = U.epoch_sprites(*args, g), U.epoch_sprites(*args, g)
    assert np.array_equal(first, a) and not np.array_equal(second, a)
    # the documented order: all glyphs, then all x0, then all y0, then all vx, then all vy
    g = _G(3)
    want = [torch.randint(0, n, (40, 3), generator=g).numpy() for n in (12, 48 - 20 + 1, 64 - 28 + 1, 11, 11)]
    for col, off in enumerate((0, 0, 0, -5, -5)):
        assert np.array_equal(a[:, :, col], want[col] + off)


def test_ranges_are_respected_and_a_single_valued_column_draws_nothing():
    t = U.epoch_sprites(4096, 2, 7, 40, 36, 28, 28, 5, _G(0))
    assert set(t[:, :, 0].ravel().tolist()) == set(range(7))
    assert t[:, :, 1].min() == 0 and t[:, :, 1].max() == 8 and t[:, :, 2].min() == 0 and t[:, :, 2].max() == 12
    assert set(t[:, :, 3].ravel().tolist()) == set(range(-5, 6)) == set(t[:, :, 4].ravel().tolist())
    U.check_sprite_table(t, 7, 40, 36, 28, 28, 5)
    # W == gw: the x0 column is all zero and nothing is drawn for it -- the stream equals one that skips the column
    g, h = _G(5), _G(5)
    t = U.epoch_sprites(16, 2, 7, 40, 28, 28, 28, 3, g)
    want = [torch.randint(0, n, (16, 2), generator=h).numpy() for n in (7, 13, 7, 7)]
    assert not t[:, :, 1].any()
    assert np.array_equal(t[:, :, 0], want[0]) and np.array_equal(t[:, :, 2], want[1])
    assert np.array_equal(t[:, :, 3], want[2] - 3) and np.array_equal(t[:, :, 4], want[3] - 3)
    assert torch.equal(torch.randint(0, 100, (4,), generator=g), torch.randint(0, 100, (4,), generator=h))
    assert U.epoch_sprites(0, 2, 7, 40, 28, 28, 28, 3).shape == (0, 2, 5)
    with pytest.raises(ValueError):
        U.epoch_sprites(4, 9, 7, 40, 40, 28, 28)                                   # D above 8
    with pytest.raises(ValueError):
        U.epoch_sprites(4, 2, 7, 20, 40, 28, 28)                                   # the glyph does not fit


@pytest.mark.parametrize("col,value,name", [(0, 12, "glyph"), (0, -1, "glyph"), (1, 37, "x0"), (1, -1, "x0"), (2, 21, "y0"),
                                            (3, 6, "vx"), (4, -6, "vy")])
def test_check_sprite_table_refuses_each_kind_of_bad_row(col, value, name):
    good = U.epoch_sprites(6, 2, 12, 48, 64, 28, 28, 5, _G(1))                     # H 48, W 64: x0 <= 36, y0 <= 20
    assert np.array_equal(U.check_sprite_table(good, 12, 48, 64, 28, 28, 5), good)
    bad = good.copy()
    bad[4, 1, col] = value
    with pytest.raises(ValueError, match=name):
        U.check_sprite_table(bad, 12, 48, 64, 28, 28, 5)
    if col < 3:                                                                    # the host mirror checks before it renders
        with pytest.raises(ValueError, match=name):
            U.render_sprites_host(np.ones((12, 28, 28), dtype=np.uint8), bad, 2, 48, 64)


def test_check_sprite_table_refuses_wrong_shapes_and_types():
    good = U.epoch_sprites(3, 2, 4, 32, 32, 8, 8, 5, _G(1))
    for bad in (good[:, :, :4], good[0], good.astype(np.float32), np.zeros((3, 9, 5), dtype=np.int32), np.zeros((3, 0, 5), dtype=np.int32)):
        with pytest.raises(ValueError):
            U.check_sprite_table(bad, 4, 32, 32, 8, 8)
    assert U.check_sprite_table(torch.from_numpy(good).long(), 4, 32, 32, 8, 8).dtype == np.int32
    fast = good.copy()
    fast[0, 0, 3] = 127                                                            # up to the kernel's own clamp by default
    U.check_sprite_table(fast, 4, 32, 32, 8, 8)
    fast[0, 0, 3] = 128
    with pytest.raises(ValueError, match="vx"):
        U.check_sprite_table(fast, 4, 32, 32, 8, 8)


# ---------------------------------------------------------------------------------------------
# glyph banks
# ---------------------------------------------------------------------------------------------
def _idx_bytes(images, magic=2051):
    n, r, c = images.shape
    return np.array([magic, n, r, c], dtype=">u4").tobytes() + images.tobytes()


def test_load_idx_images_round_trips_plain_and_gz_and_refuses_a_bad_magic(tmp_path):
    images = np.random.default_rng(0).integers(0, 256, (5, 7, 9), dtype=np.uint8)
    plain, packed = tmp_path / "images-idx3-ubyte", tmp_path / "images-idx3-ubyte.gz"
    plain.write_bytes(_idx_bytes(images))
    with gzip.open(packed, "wb") as f:
        f.write(_idx_bytes(images))
    for p in (plain, packed):
        got = U.load_idx_images(p)
        assert got.dtype == np.uint8 and got.flags.writeable and np.array_equal(got, images)
    labels = tmp_path / "labels-idx1-ubyte"
    labels.write_bytes(_idx_bytes(images, magic=2049))
    with pytest.raises(ValueError, match="2051"):
        U.load_idx_images(labels)
    short = tmp_path / "short-idx3-ubyte"
    short.write_bytes(_idx_bytes(images)[:-3])
    with pytest.raises(ValueError):
        U.load_idx_images(short)
    tiny = tmp_path / "tiny"
    tiny.write_bytes(b"\0\0\10")
    with pytest.raises(ValueError):
        U.load_idx_images(tiny)


def test_procedural_glyphs_match_the_recorded_checksum(golden):
    bank = U.procedural_glyphs(12, 28, seed=0)
    assert bank.dtype == np.uint8 and bank.shape == (12, 28, 28)
    assert np.array_equal(bank, golden["bank"])                                    # the bank the reference run was fed
    assert hashlib.sha256(bank.tobytes()).hexdigest() == PROCEDURAL_SHA256
    assert np.array_equal(bank, U.procedural_glyphs(12, 28, seed=0)) and not np.array_equal(bank, U.procedural_glyphs(12, 28, seed=1))
    assert np.array_equal(U.procedural_glyphs(3, 28, seed=0), bank[:3])
    # glyph-like: a background margin, a solid stroke, nothing faint
    assert bank.max() == 255 and not bank[:, 0].any() and not bank[:, :, -1].any()
    cover = (bank > 0).mean(axis=(1, 2))
    assert cover.min() > 0.03 and cover.max() < 0.6 and bank[bank > 0].min() >= 51
    odd = U.procedural_glyphs(2, 12, seed=3)
    assert odd.shape == (2, 12, 12) and odd.any()
    with pytest.raises(ValueError):
        U.procedural_glyphs(2, 65)


# ---------------------------------------------------------------------------------------------
# loader and C ABI without a device
# ---------------------------------------------------------------------------------------------
def test_loader_on_the_cpu_is_an_error():
    with pytest.raises(U.UclstmError, match="HIP device"):
        U.DeviceSpriteLoader(U.procedural_glyphs(2), 2, 3, device="cpu")


def test_entry_point_is_declared_exported_and_bound():
    with open(L.HEADER_PATH) as f:
        hdr = f.read()
    assert RENDER in L.header_symbols() and RENDER in L._PROTOS and RENDER not in L.F16_TWINS
    assert re.search(r"int32_t\s+uclstm_sprites_render\(const uint8_t\* bank,", hdr)
    # an additive change: one new entry point, the ABI version the header, the binding and the library agree on is unchanged
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == int(re.search(r"#define UCLSTM_ABI_VERSION\s+(\d+)", hdr).group(1))
    raw = C.CDLL(L.LIB_PATH)
    assert hasattr(raw, RENDER) and not hasattr(raw, RENDER + "_f16")
    assert len(L._PROTOS[RENDER]) == 17
    from unet_convlstm_amd import build as B
    assert "sprites.hip" in B.SOURCES and "sprites.hip" not in B.F16_SOURCES


def _call(**over):
    """uclstm_sprites_render with fake non-NULL pointers: every case below must be refused BEFORE anything is launched."""
    a = dict(bank=0x1000, n_glyph=4, gh=28, gw=28, table=0x2000, n_out=2, D=2, T=3, C=2, H=64, W=64, v_scale=5.0,
             x=0x10000, y=0x20000, mask=0x30000, raw=None, stream=None)
    a.update(over)
    return L.lib.uclstm_sprites_render(*(a[k] for k in ("bank", "n_glyph", "gh", "gw", "table", "n_out", "D", "T", "C", "H", "W",
                                                       "v_scale", "x", "y", "mask", "raw", "stream")))


@pytest.mark.parametrize("over", [dict(gw=65, W=128), dict(gh=65, H=128), dict(gw=40, W=36), dict(gh=40, H=36), dict(D=0), dict(D=9),
                                  dict(T=0), dict(bank=None), dict(table=None), dict(x=None), dict(y=None), dict(mask=None),
                                  dict(n_glyph=0), dict(n_out=0), dict(C=0), dict(gh=0), dict(gw=0), dict(v_scale=0.0),
                                  dict(n_out=1 << 20, T=64, H=64, W=64)])
def test_entry_point_refuses_bad_arguments_before_launching(over):
    assert _call(**over) == -1
