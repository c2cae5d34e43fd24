"""The valid-pixel walk of the 256 x 256 weight-gradient kernels (csrc/igemm_wgrad.hip, csrc/wgrad_walk.h): a tile whose columns
belong to one tap reduces over the pixels whose tap falls inside the image only, and each pixel range owns a share of the tap's own
K-tiles.  Slab mode, both 16-bit types, called at the C ABI like tests/test_gpu_wgrad_abi.py and held to the same criterion:
every element of every slab written and finite between intact guard zones, structural zeros exactly 0, the f64 sum of the slabs
within coeff(c, splits) * mag of wgrad_cases.wgrad_ref.

UCLSTM_WGRAD_VALID is read once per process, so the dense arm (UCLSTM_WGRAD_VALID=0) runs in one child process that writes its
slabs to a temporary .npz.  The centre tap visits every pixel either way, range by range the same K-tiles in the same order: its
columns must agree bit for bit between the arms.  A 1x1 gradient has no padded tap and must agree bit for bit as a whole.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wgrad_cases as WC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import test_gpu_wgrad_abi as T

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _case(n_img, C0, C1, Co, H, W, ktap=3, pad=1):
    name = f"V-{n_img}x{H}x{W}-{C0}+{C1}-{Co}-k{ktap}"
    return WC.WCase(name, 3, n_img, H, W, [(c, H, W, 0, 0) for c in (C0, C1) if c], Co, ktap=ktap, pad=pad)


def _smallest_image():
    """The smallest image the shape query still sends to the 256 x 256 kernel (64 pixels in all, one K-tile of the dense walk)."""
    for H, W in ((1, 1), (1, 2), (2, 2), (2, 4)):
        c = _case(64 // (H * W), 256, 0, 256, H, W)
        if WC.wgrad_shape(WC.build_wgrad_desc(c)) == 3:
            return c
    raise AssertionError("no image up to 2 x 4 reaches the 256 x 256 kernel")


# (case, explicit splits)
def _jobs():
    return [
        (_case(4, 256, 0, 256, 4, 4), 1),            # one K-tile: corner taps fill 36 of its 64 rows
        (_case(8, 256, 0, 256, 4, 4), 1),
        (_case(20, 256, 256, 1024, 4, 4), 1),        # five dense K-tiles, three of a corner tap, four of an edge tap
        (_case(20, 256, 256, 1024, 4, 4), 3),
        (_case(20, 256, 256, 1024, 4, 4), 5),        # ranges 3 and 4 store zero tiles for the corner taps
        (_case(6, 256, 0, 256, 8, 8), 2),
        (_case(2, 256, 0, 512, 16, 16), 3),
        (_case(2, 256, 0, 256, 64, 64), 4),          # W >= 64; rows of the walk cross stage boundaries
        (_case(8, 256, 0, 256, 2, 4), 1),
        (_smallest_image(), 1),                      # 1 x 1: eight taps never fall inside the image
        (_case(8, 256, 0, 256, 4, 4, ktap=1, pad=0), 1),      # no padded tap: the dense walk in both arms
    ]


def job_ids():
    return [f"{c.name}-s{s}" for c, s in _jobs()]


@functools.lru_cache(maxsize=32)
def operands(name, tag):
    c = next(c for c, _ in _jobs() if c.name == name)
    xs, dys = WC.make_operands(c, DTYPES[tag])
    ref, mag = WC.case_ref(c, xs, dys)
    return c, [x.cuda().contiguous() for x in xs], [t.cuda().contiguous() for t in dys], ref, mag


def run(c, xd, dyd, splits, dtype):
    """Launch in slab mode into a guarded buffer -> (slabs [used][N][Ktot] f64, mask of untouched elements of the whole buffer, used)."""
    panel = c.N * c.Ktot
    d = T.desc_of(c, xd, dyd, splits=splits, slab=panel)
    assert WC.wgrad_shape(d) == 3, c.name
    used = WC.wgrad_splits(d)
    assert 1 <= used <= splits
    d.splits = used
    assert WC.wgrad_splits(d) == used
    buf = T.Guarded(used + 1, panel)
    d.dwp = buf.ptr()
    assert T.launch(d, dtype) == 0, c.name
    got, untouched = buf.read()
    return got[:used].reshape(used, c.N, c.Ktot), untouched, used


def tap_columns(c, tap):
    kseg = sum(c.ksegs)
    return slice(tap * kseg, (tap + 1) * kseg)


RESULTS = {}       # (job id, type tag) -> slabs of this process (walk on), float32 bits


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("job", range(len(job_ids())), ids=job_ids())
def test_valid_walk_against_f64(job, tag):
    c0, splits = _jobs()[job]
    c, xd, dyd, ref, mag = operands(c0.name, tag)
    slabs, untouched, used = run(c, xd, dyd, splits, DTYPES[tag])
    what = f"{c.name} splits {splits} {tag}"
    expect = torch.ones_like(untouched)
    expect[:used] = False
    assert bool((untouched == expect).all()), f"{what}: {int((untouched & ~expect).sum())} slab elements not written"
    assert bool(torch.isfinite(slabs).all()), what
    assert bool((slabs[:, mag == 0] == 0).all()), f"{what}: a structural zero of some slab is not exactly 0"
    T.check_panel(slabs.sum(0), ref, mag, None, T.coeff(c, used), DTYPES[tag], f"{what} ({used} slabs)", 3)
    if c.ktap == 3:
        # a range beyond the tap's own K-tiles stores a tile of zeros (that the walk is on at all shows here)
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            rows = c.n_img * max(c.H - abs(dy), 0) * max(c.W - abs(dx), 0)
            ktiles = -(-rows // 64)
            per = -(-ktiles // used) if ktiles else 0
            for r in range(used):
                if per == 0 or r * per >= ktiles:
                    assert bool((slabs[r][:, tap_columns(c, tap)] == 0).all()), f"{what}: range {r} of tap {tap} owns no K-tile and is not zero"
        if (c.n_img, c.H, c.W, splits) == (20, 4, 4, 5):
            assert bool((slabs[3:][:, :, tap_columns(c, 0)] == 0).all()) and bool((slabs[2][:, tap_columns(c, 0)] != 0).any())
            assert bool((slabs[4][:, tap_columns(c, 4)] != 0).any())
    RESULTS[(job_ids()[job], tag)] = slabs.float().numpy().view(np.uint32)


def child_main(out):
    res = {}
    for tag, dtype in DTYPES.items():
        for (c0, splits), jid in zip(_jobs(), job_ids()):
            c, xd, dyd, _, _ = operands_no_ref(c0, tag)
            slabs, _, _ = run(c, xd, dyd, splits, dtype)
            res[f"{jid}|{tag}"] = slabs.float().numpy().view(np.uint32)
    np.savez(out, **res)


def operands_no_ref(c, tag):
    xs, dys = WC.make_operands(c, DTYPES[tag])
    return c, [x.cuda().contiguous() for x in xs], [t.cuda().contiguous() for t in dys], None, None


CHILD = "import sys; sys.path[:0] = sys.argv[1:3]; import test_gpu_wgrad_valid as V; V.child_main(sys.argv[3])"


def test_dense_arm_agrees_bit_for_bit_on_the_centre_tap(tmp_path):
    """UCLSTM_WGRAD_VALID=0 in a child: centre-tap columns of every slab equal this process's, the 1x1 gradient as a whole, and the
    padded taps of the dense arm meet the same f64 bound (it is the A/B arm of the measurements)."""
    for jid in job_ids():
        for tag in DTYPES:
            if (jid, tag) not in RESULTS:
                test_valid_walk_against_f64(job_ids().index(jid), tag)
    out = str(tmp_path / "dense.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("UCLSTM_WGRAD_")}
    env["UCLSTM_WGRAD_VALID"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT_DIR, os.path.join(ROOT_DIR, "tests"), out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"child failed ({r.returncode}): {r.stderr[-3000:]}"
    dense = np.load(out)
    bad = []
    differs = 0
    for (c, splits), jid in zip(_jobs(), job_ids()):
        for tag in DTYPES:
            a, b = RESULTS[(jid, tag)], dense[f"{jid}|{tag}"]
            assert a.shape == b.shape, (jid, tag)
            if c.ktap == 1:
                if not np.array_equal(a, b):
                    bad.append(f"{jid} {tag}: the 1x1 gradient differs between the arms")
                continue
            cols = tap_columns(c, 4)
            if not np.array_equal(a[:, :, cols], b[:, :, cols]):
                bad.append(f"{jid} {tag}: {int((a[:, :, cols] != b[:, :, cols]).sum())} centre-tap elements differ between the arms")
            differs += int(not np.array_equal(a, b))
            _, _, _, ref, mag = operands(c.name, tag)
            used = a.shape[0]
            T.check_panel(torch.from_numpy(b.view(np.float32)).double().sum(0), ref, mag, None, T.coeff(c, used), DTYPES[tag],
                          f"{jid} dense arm ({used} slabs)", 3)
    assert not bad, "\n".join(bad)
    assert differs > 0, "the arms agree everywhere: the switch does nothing"
