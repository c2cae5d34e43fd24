"""Dispatch plan of the flat forward kernel (no GPU: validation-only entry points, dummy aligned pointers): every case of
tests/flat_cases.py reports kernel 4, every near miss the kernel it took before, the statistics rows are the rows
uclstm_igemm_tiles_per_group promises (128 pixels for N > 64, else 256), and UCLSTM_FWD_FLAT=0 (read once per process) sends
every case back to the per-tap loop."""
import ctypes as C
import os
import subprocess
import sys

import flat_cases as FC
import igemm_cases as IC

L = IC.L
ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shape(c):
    return int(L.lib.uclstm_igemm_fwd_shape(C.byref(IC.dummy_desc(c))))


def test_flat_cases_report_the_flat_kernel():
    names = [c.name for c in FC.FLAT_CASES]
    assert len(set(names)) == len(names)
    for c in FC.FLAT_CASES:
        assert c.shape == 4 and shape(c) == 4, c.name
        assert c.epi == L.EPI_STORE and len(c.srcs) == 1 and (c.srcs[0][0] % 64 == 0 or c.srcs[0][0] < 64) and (c.M // c.groups) % 256 == 0, c.name
    # the mechanisms the table is there for: K-steps 1, 2, 4, 5; zero panel rows; both gathers; more tiles than blocks
    assert {c.Ktot // 64 for c in FC.FLAT_CASES} >= {1, 2, 4, 5}
    assert any(c.N % 128 for c in FC.FLAT_CASES) and {c.ktap for c in FC.FLAT_CASES} == {1, 2}
    assert sum(c.M // 256 > 256 and -(-c.N // 128) == 1 for c in FC.FLAT_CASES) == 2


def test_near_misses_keep_their_kernel():
    for c, why in FC.NEAR_MISSES:
        assert c.shape in (0, 1) and shape(c) == c.shape, f"{c.name} ({why})"


def test_statistics_rows_are_the_rows_of_the_per_tap_shapes():
    for c in FC.FLAT_CASES:
        if c.stats:
            tiles = IC.stats_tiles(c)
            assert len(tiles) == c.groups * L.lib.uclstm_igemm_tiles_per_group(c.n_img, c.H, c.W, c.groups, c.N), c.name
            assert all(len(p) == (128 if c.N > 64 else 256) for p in tiles), c.name


def test_switch_routes_everything_back_to_the_per_tap_loop():
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import ctypes as C, flat_cases as FC, igemm_cases as IC\n"
            "print([int(IC.L.lib.uclstm_igemm_fwd_shape(C.byref(IC.dummy_desc(c)))) for c in FC.FLAT_CASES])\n"
            % (ROOT_DIR, os.path.join(ROOT_DIR, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UCLSTM_FWD_FLAT="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == str([0 if c.N > 64 else 1 for c in FC.FLAT_CASES])
