"""The valid-pixel walk of the 256 x 256 weight-gradient kernels (csrc/wgrad_walk.h) through its host query
uclstm_igemm_wgrad_walk, against a brute-force enumeration: for every tap of a 3x3 / pad 1 gradient the output pixels whose source
pixel lies inside the image, image by image and row by row.  No GPU: the query runs the inline function the kernels stage with.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from unet_convlstm_amd import _lib as L

SIZES = [1, 2, 4, 8, 16, 64]
E_BADARG = -1


def desc(n_img, H, W, ktap=3, pad=1):
    d = L.WgradDesc()
    d.n_img, d.H, d.W, d.ktap, d.pad, d.scale = n_img, H, W, ktap, pad, 1
    return d


def walk(d, tap, i0, n):
    out = (C.c_int32 * max(n, 1))()
    total = int(L.lib.uclstm_igemm_wgrad_walk(C.byref(d), tap, i0, n, out))
    return total, np.frombuffer(out, dtype=np.int32, count=n).copy()


def brute(n_img, H, W, tap, ktap=3, pad=1):
    """Pixel indices, in walk order, whose source pixel of this tap is inside the image."""
    dy, dx = tap // ktap - pad, tap % ktap - pad
    out = []
    for img in range(n_img):
        for y in range(H):
            for x in range(W):
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    out.append((img * H + y) * W + x)
    return np.asarray(out, dtype=np.int64)


@pytest.mark.parametrize("n_img", [1, 5])
@pytest.mark.parametrize("H,W", list(itertools.product(SIZES, SIZES)))
def test_walk_matches_brute_force(H, W, n_img):
    d = desc(n_img, H, W)
    for tap in range(9):
        want = brute(n_img, H, W, tap)
        dy, dx = tap // 3 - 1, tap % 3 - 1
        hv, wv = max(H - abs(dy), 0), max(W - abs(dx), 0)
        assert len(want) == n_img * hv * wv
        # the whole walk and 70 entries past its end
        total, got = walk(d, tap, 0, len(want) + 70)
        assert total == n_img * hv * wv, (tap, total)
        assert np.array_equal(got[:total], want), tap
        assert (got[total:] == -1).all(), tap
        # ranges that start inside an image / a row and cross the boundaries: the 64-row stages of the kernels among them
        nv = hv * wv
        for i0, n in {(0, 0), (1, 64), (max(wv - 1, 0), 3), (max(nv - 2, 0), 5), (64, 64), (max(total - 3, 0), 64), (total, 4), (total + 9, 2)}:
            t2, seg = walk(d, tap, i0, n)
            assert t2 == total
            ref = np.full(n, -1, dtype=np.int64)
            k = max(0, min(n, total - i0))
            ref[:k] = want[i0:i0 + k]
            assert np.array_equal(seg, ref), (tap, i0, n)


def test_walk_of_images_that_are_no_power_of_two():
    """The query is not restricted to the kernels' shapes: general multiplies instead of shifts."""
    for n_img, H, W in ((3, 9, 11), (2, 3, 5), (4, 1, 7)):
        d = desc(n_img, H, W)
        for tap in range(9):
            want = brute(n_img, H, W, tap)
            total, got = walk(d, tap, 0, len(want) + 3)
            assert total == len(want) and np.array_equal(got[:total], want) and (got[total:] == -1).all(), (H, W, tap)


def test_walk_rejects_bad_arguments():
    d = desc(2, 4, 4)
    buf = (C.c_int32 * 4)()
    f = L.lib.uclstm_igemm_wgrad_walk
    assert f(None, 0, 0, 4, buf) == E_BADARG
    assert f(C.byref(d), 9, 0, 4, buf) == E_BADARG and f(C.byref(d), -1, 0, 4, buf) == E_BADARG
    assert f(C.byref(d), 0, -1, 4, buf) == E_BADARG and f(C.byref(d), 0, 0, -1, buf) == E_BADARG
    assert f(C.byref(d), 0, 0, 4, None) == E_BADARG
    assert f(C.byref(d), 4, 0, 0, None) == 2 * 16
    assert f(C.byref(desc(0, 4, 4)), 0, 0, 4, buf) == E_BADARG
