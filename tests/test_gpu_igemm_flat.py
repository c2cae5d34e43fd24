"""The flat forward kernel (csrc/igemm_fwd.hip, igemm_fwd_flat_kernel: persistent 128 x 256 tiles, a three-stage ring over all
the tiles of a block, epilogue from registers) at the C ABI, in bf16 and fp16.  Every case of tests/flat_cases.py, three ways:

  * against the host f64 reference with the bounds of test_gpu_igemm_abi.test_store_epilogue_against_f64 (its own checkers are
    reused): every destination between NaN-pattern guard zones, every statistics slot against the kernel's own stored values;
  * bit for bit against the same descriptors on the per-tap loop (UCLSTM_FWD_FLAT=0, read once per process, so a fresh child
    process): the kernel walks K in the per-tap loop's order with the same MFMA sequence; the statistics differ in their f32
    summation order only (the tolerance test_gpu_ops uses for the patch loop against the per-tap loop);
  * eight launches of the same descriptor in one process give identical bytes (a screen for ring hazards: a comparison of
    what eight launches wrote, never a retry).
The two runner processes (one per dtype and switch value) are started once per module and shared.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import flat_cases as FC
import igemm_cases as IC
import test_gpu_igemm_abi as AB

pytestmark = pytest.mark.gpu

L = IC.L
ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
NAMES = [c.name for c in FC.FLAT_CASES]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(dtype name, switch): result of flat_cases.run_all}: "1" in this process, "0" (per-tap loop) in a child per dtype."""
    cache = {}

    def get(dtype, switch):
        name = str(dtype).split(".")[-1]
        if (name, switch) not in cache:
            f = str(tmp_path_factory.mktemp("flat") / f"{name}_{switch}.pt")
            if switch == "1":
                FC.run_all(name, f)
            else:
                code = ("import sys; sys.path[:0] = [%r, %r]\nimport flat_cases\nflat_cases.run_all(sys.argv[1], sys.argv[2])\n"
                        % (ROOT_DIR, os.path.join(ROOT_DIR, "tests")))
                r = subprocess.run([sys.executable, "-c", code, name, f], env=dict(os.environ, UCLSTM_FWD_FLAT=switch), capture_output=True,
                                   text=True, timeout=300)
                assert r.returncode == 0, r.stderr[-2500:]
            cache[(name, switch)] = torch.load(f)
        return cache[(name, switch)]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=AB.tag)
@pytest.mark.parametrize("name", NAMES)
def test_flat_kernel_against_f64(name, dtype):
    c = next(x for x in FC.FLAT_CASES if x.name == name)
    xd, wp, (xs, bias, col_scale, col_shift), keep = FC.operands(c, dtype)
    A = IC.gather_a(c.n_img, c.H, c.W, c.ktap, c.scale, c.pad, [(x, s[3], s[4]) for x, s in zip(xs, c.srcs)])
    ref, mag = IC.gemm_ref(A, wp.cpu())
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if c.affine:
        ref = ref * col_scale.double() + col_shift.double()
        mag = mag * col_scale.double().abs() + col_shift.double().abs()
    if c.relu:
        ref = ref.clamp(min=0.0)
    segs = c.segments()
    outs = [AB.Guarded((c.n_img, s[4], s[5], s[2]), dtype) for s in segs]
    tiles = IC.stats_tiles(c) if c.stats else None
    stats = AB.Guarded((len(tiles), c.N, 2), torch.float32) if c.stats else None
    d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), [o.ptr() for o in outs],
                      *[None if t is None else t.data_ptr() for t in keep], stats.ptr() if stats else None)
    AB.assert_shape(c, d)
    AB.launch(d, dtype, name)
    refs, mags = IC.scatter_segments(ref, c.n_img, c.H, c.W, segs), IC.scatter_segments(mag, c.n_img, c.H, c.W, segs)
    for i, o in enumerate(outs):
        got, untouched = o.read()
        AB.check_16bit(got, untouched, refs[i], mags[i], dtype, f"{name} segment {i}", "STORE kernel 4")
        assert int((~untouched).sum()) > 0
    if c.stats:
        assert len(segs) == 1 and segs[0][6:] == (1, 0, 0) and segs[0][3] == 0 and segs[0][:2] == (0, c.N)
        stored = outs[0].read()[0].view(c.M, segs[0][2])[:, :c.N]
        sgot, suntouched = stats.read()
        assert not bool(suntouched.any()), f"{name}: statistics slots not written"
        sref = torch.stack([torch.stack((stored[p].sum(0), (stored[p] ** 2).sum(0)), -1) for p in tiles])
        sabs = torch.stack([torch.stack((stored[p].abs().sum(0), (stored[p] ** 2).sum(0)), -1) for p in tiles])
        e = float(((sgot - sref).abs() / (sabs + 1e-30)).max())
        print(f"[parity] {name} stats {AB.tag(dtype)}: max |err| / sum|terms| {e:.2e} (<= 2e-6) over {sref.numel()} sums")
        AB.note("stats kernel 4", dtype, e / 2e-6)
        assert e <= 2e-6, f"{name}: statistics slot off by {e:.3e} of sum|terms|"


@pytest.mark.parametrize("dtype", DTYPES, ids=AB.tag)
def test_flat_kernel_is_bit_identical_to_the_per_tap_loop(runs, dtype):
    flat, pertap = runs(dtype, "1"), runs(dtype, "0")
    for name in NAMES:
        N = next(c.N for c in FC.FLAT_CASES if c.name == name)
        assert flat[name]["shape"] == 4 and pertap[name]["shape"] == (0 if N > 64 else 1), name
        for i, (a, b) in enumerate(zip(flat[name]["out"][0], pertap[name]["out"][0])):
            assert bool((a != 0x7FE5).any()), name
            assert torch.equal(a, b), f"{name} segment {i}: {int((a != b).sum())} of {a.numel()} 16-bit words differ"
        if flat[name]["stats"][0] is not None:
            s, r = flat[name]["stats"][0], pertap[name]["stats"][0]
            assert bool(torch.isfinite(s).all()), name
            torch.testing.assert_close(s, r, rtol=1e-4, atol=1e-2, msg=name + " stats")


@pytest.mark.parametrize("dtype", DTYPES, ids=AB.tag)
def test_repeated_launches_give_identical_bytes(runs, dtype):
    flat = runs(dtype, "1")
    for name in NAMES:
        rec = flat[name]
        assert len(rec["out"]) == FC.REPEATS == 8
        for k in range(1, FC.REPEATS):
            for a, b in zip(rec["out"][0], rec["out"][k]):
                assert torch.equal(a, b), f"{name}: launch {k} differs from launch 0 in {int((a != b).sum())} words"
            if rec["stats"][0] is not None:
                assert torch.equal(rec["stats"][0], rec["stats"][k]), f"{name}: statistics of launch {k} differ"
