"""The forward MFMA loops after their LDS fragment reads were moved one step ahead of the MFMAs that consume them
(csrc/igemm_fwd.hip: the ring kernel's 18-step tile body and the two 32-deep halves of a patch-loop K-step).

The arithmetic did not move -- the order of MFMAs per accumulator is what it was -- so every output must stay BIT-IDENTICAL to the
kernel the same launch takes with the loop switched off: the ring kernel against UCLSTM_FWD_C64=0, the patch loop against
UCLSTM_FWD_PATCH=0 (the per-tap loop, which has no second fragment set).  The switches are read once per process, so each arm is a
process of its own (tests/fwd_read_pipeline_cases.py; the pattern of tests/test_gpu_ops.py).  BatchNorm partial sums are compared to
the tolerances of that file (f32 summation order).  What a too-early read would show as: a fragment of the previous tile's / step's
slot, or of a row the DMA has not landed -- wrong values in some tiles, not a crash; hence shapes where slots are reused at once
(three tiles per block, one tile per image, odd chunk counts, a source switch at a chunk boundary, one chunk per split-K range).

So that both arms cannot be wrong together, every output of the new arm is also checked once against an f64 reference at the bounds
of tests/test_gpu_igemm_abi.py (computed in the launching process, see there); the worst |err| / bound comes back with the outputs.

Two of the listed shapes cannot reach the patch loop and say so in the case table: a one-chunk STORE launch (K = 576) and a pixel
count that is no multiple of 256 are routed to the per-tap loop by the library in both arms.  They stay as cases -- the routing is
part of what is compared -- and the one-chunk path of the patch loop (`more` false from the first tap, `vmcnt(0)`) is reached by
the split-K case, whose K ranges are one chunk each.
"""
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import fwd_read_pipeline_cases as FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["bfloat16", "float16"]
SWITCH = {"ring": "UCLSTM_FWD_C64", "patch": "UCLSTM_FWD_PATCH"}
PATCH_NAMES = [c[0] for c in FC.STORE_CASES] + [FC.SLAB_CASE[0], "lstm_4x4", "group_of_two"]
# kernel the library reports per launch of a case with the loop ON (3 ring, 2 patch loop, 0 / 1 per-tap shapes)
EXPECT_ON = {**{c[0]: [3] for c in FC.RING_CASES}, **{c[0]: [c[7]] for c in FC.STORE_CASES}, FC.SLAB_CASE[0]: [2], "lstm_4x4": [2],
             "group_of_two": [2, 2]}


@functools.lru_cache(maxsize=None)
def arms(family, dtype):
    """(new, old): the results of all cases of a family with its loop on (and the f64 check) and off; one process each."""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for val in ("1", "0"):
            f = os.path.join(tmp, val + ".pt")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fwd_read_pipeline_cases.py"), f, dtype, family, val],
                               env=dict(os.environ, **{SWITCH[family]: val}), capture_output=True, text=True, timeout=240)
            assert r.returncode == 0, r.stderr[-2500:]
            out.append(torch.load(f))
    return tuple(out)


def compare(family, dtype, name):
    new, old = (a[name] for a in arms(family, dtype))
    assert new["shapes"] == EXPECT_ON[name], f"{name}: launched as kernel {new['shapes']}"
    assert (3 if family == "ring" else 2) not in old["shapes"], f"{name}: the reference arm ran kernel {old['shapes']}"
    for k, v in new.items():
        if k in ("shapes", "worst"):
            continue
        assert bool(torch.isfinite(v.float()).all()), f"{name}.{k}: elements not written"
        if k == "stats":
            torch.testing.assert_close(v, old[k], rtol=1e-4, atol=1e-2, msg=f"{name}.{k}")
        else:
            assert torch.equal(v, old[k]), f"{name}.{k}: max abs diff {float((v.float() - old[k].float()).abs().max())}"
    for k, w in new["worst"].items():
        print(f"[parity] {family} {name}.{k} {dtype}: worst |err| / bound against f64 {w:.3f} (<= 1)")
    for k, w in new["worst"].items():
        assert w <= 1.0, f"{name}.{k}: {w:.3f} x the f64 bound"
    assert float(next(v for k, v in new.items() if k not in ("shapes", "worst", "stats")).float().abs().max()) > 0.05


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c[0] for c in FC.RING_CASES])
def test_ring_kernel_is_bit_identical_with_its_reads_a_step_ahead(name, dtype):
    compare("ring", dtype, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", PATCH_NAMES)
def test_patch_loop_is_bit_identical_with_its_second_half_read_ahead(name, dtype):
    compare("patch", dtype, name)
