"""The weight-gradient GEMM family (csrc/igemm_wgrad.hip: generic addressing in its PLAIN and non-PLAIN instantiation, the
buffer-addressed power-of-two kernel with 64x256 / 64x192 / 128x128 tiles, the 256x256 kernel, the ring-staged 64 -> 64 kernel;
slab and atomic mode, automatic / explicit / overlapped split plans) called directly at the C ABI with hand-built descriptors,
in bf16 and fp16, and compared element by element with a host f64 reference that restates the contract of include/uclstm.h
(tests/wgrad_cases.py; pinned to PyTorch's f64 autograd by tests/test_cabi_and_host.py).

The operands are randn * 0.8 rounded to the 16-bit type on the host; the reference multiplies exactly those values, so the only
differences are f32 accumulation and the f32 adds of the partial panels:
    |err| <= c * (mag + |P|) + 1e-30,   c = max(2e-6, (M/32 + splits + 2) * 2^-24),   M = n_img*H*W
one f32 rounding per MFMA accumulation step (32 pixels each) plus one per added partial (the host adds the slabs in f64, the atomics
round once each); mag = |dY|^T |A|, P = the panel pre-loaded in atomic mode (0 in slab mode).  The LDS-staged epilogues move f32
values and add no rounding.  Where mag == 0 (padding columns of a 64-channel K segment, rows no segment covers) every slab must
hold exactly 0 and an atomic launch must leave exactly P.  Nothing is excluded.

dwp sits in a buffer pre-filled with a NaN bit pattern, between guard zones of the same pattern and followed by one spare slab:
in slab mode every element of every one of the uclstm_igemm_wgrad_splits() slabs must be written and finite, and the guards,
the spare slab and the gap between slabs (slab > N*Ktot) must still hold the pattern.  How pixels are divided among the slabs is
the library's business (the ring kernel divides tiles, not pixel ranges), so the SUM of the slabs is compared.

Every case asserts the kernel it is meant for through uclstm_igemm_wgrad_shape before it launches.  UCLSTM_WGRAD_GENERIC is read
once per process: the last test runs three power-of-two cases through the generic kernel in one child process.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

import wgrad_cases as WC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_convlstm_amd import ops

L = WC.L
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
PATTERN = 0x7FC07FE5             # a NaN in f32
GUARD = 4096                     # elements before and after the buffer
E_BADARG = -1                    # UCLSTM_E_BADARG
WORST = {}                       # (kernel, dtype tag) -> worst |err| / bound, printed when the module is done
ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """After the module's last test: the worst measured |err| / bound of every kernel (the DESIGN.md table; run with -s)."""
    yield
    print_summary()


def print_summary():
    for (what, t), v in sorted(WORST.items()):
        print(f"[parity-summary] {what} {t}: {v:.3e}")


def tag(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def coeff(c, splits):
    return max(2e-6, (c.M / 32 + splits + 2) * 2.0 ** -24)


class Guarded:
    """A device f32 buffer [rows][cols] between two guard zones, all filled with a NaN bit pattern."""

    def __init__(self, rows, cols):
        self.rows, self.cols, self.n = rows, cols, rows * cols
        self.raw = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.n].view(torch.float32).view(rows, cols)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def load(self, x):
        self.t.copy_(x.float().view(self.rows, self.cols))

    def read(self):
        """(values as f64 on the host, mask of elements that still hold the pattern); asserts the guards are intact."""
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + self.n:] == PATTERN).all()), "write outside the buffer"
        body = raw[GUARD:GUARD + self.n].view(self.rows, self.cols)
        return body.view(torch.float32).double(), body == PATTERN


@functools.lru_cache(maxsize=4)
def prepared(name, dtype):
    """The case, its operands on the device and its f64 reference (computed once per case and type, never modified)."""
    c = WC.case(name)
    xs, dys = WC.make_operands(c, dtype)
    ref, mag = WC.case_ref(c, xs, dys)
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all()) and float((mag > 0).double().mean()) > 0.02
    return c, [x.to(DEV).contiguous() for x in xs], [t.to(DEV).contiguous() for t in dys], ref, mag


def desc_of(c, xd, dyd, **kw):
    return WC.build_wgrad_desc(c, [x.data_ptr() for x in xd], [t.data_ptr() for t in dyd], **kw)


def launch(d, dtype):
    rc = int(L.kernels(dtype).uclstm_igemm_wgrad(C.byref(d), ops._stream()))
    torch.cuda.synchronize()
    return rc


def check_panel(got, ref, mag, pre, coef, dtype, what, kernel):
    """Every element of a panel [N][Ktot]: |got - (pre + ref)| <= coef * (mag + |pre|) + 1e-30."""
    base = torch.zeros_like(ref) if pre is None else pre.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: elements not written"
    bound = coef * (mag + base.abs()) + 1e-30
    d = (got - (ref + base)).abs()
    worst = float((d / bound).max())
    print(f"[parity] {what} {tag(dtype)}: kernel {kernel}, worst |err| / bound {worst:.3f} (<= 1), max |err| {float(d.max()):.3e} over "
          f"{d.numel()} elements, {int((mag == 0).sum())} of them structural zeros")
    key = (f"wgrad kernel {kernel}", tag(dtype))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    bad = int((d > bound).sum())
    assert bad == 0, f"{what}: {bad} of {d.numel()} elements beyond the bound (worst {worst:.3f} x)"


def run_slabs(name, dtype, what, kernel=None, splits=0, overlapped=0, accumulate=0, gap=0):
    """Slab mode: query, launch with the answer, the write contract, then the f64 sum of the slabs against the reference.
    -> (slabs [used][N][Ktot] f64, used)"""
    c, xd, dyd, ref, mag = prepared(name, dtype)
    kernel = c.shape if kernel is None else kernel
    panel = c.N * c.Ktot
    d = desc_of(c, xd, dyd, splits=splits, overlapped=overlapped, accumulate=accumulate, slab=panel + gap)
    assert WC.wgrad_shape(d) == kernel, f"{what}: dispatches to kernel {WC.wgrad_shape(d)}, meant for {kernel}"
    used = WC.wgrad_splits(d)
    assert used >= 1 and (splits == 0 or used <= splits), f"{what}: {used} slabs for splits = {splits}"
    d.splits = used
    assert WC.wgrad_splits(d) == used, f"{what}: the slab count is not stable"
    buf = Guarded(used + 1, panel + gap)
    d.dwp = buf.ptr()
    assert launch(d, dtype) == 0, what
    got, untouched = buf.read()
    expect = torch.ones_like(untouched)
    expect[:used, :panel] = False
    n_bad = int((untouched != expect).sum())
    assert n_bad == 0, (f"{what}: {int((untouched & ~expect).sum())} slab elements not written, {int((~untouched & expect).sum())} "
                        f"elements written beyond the {used} slabs")
    slabs = got[:used, :panel].reshape(used, c.N, c.Ktot)
    assert bool(torch.isfinite(slabs).all()), f"{what}: non-finite values stored"
    assert bool((slabs[:, mag == 0] == 0).all()), f"{what}: a structural zero of some slab is not exactly 0"
    check_panel(slabs.sum(0), ref, mag, None, coeff(c, used), dtype, f"{what} ({used} slabs)", kernel)
    return slabs, used


def run_atomic(name, dtype, what, kernel=None, splits=0):
    """Atomic mode onto a random pre-loaded panel P: the result against P + reference, exactly P where mag == 0."""
    c, xd, dyd, ref, mag = prepared(name, dtype)
    kernel = c.shape if kernel is None else kernel
    pre = torch.randn(c.N, c.Ktot, generator=torch.Generator().manual_seed(11))
    d = desc_of(c, xd, dyd, splits=splits, slab=0)
    assert WC.wgrad_shape(d) == kernel, f"{what}: dispatches to kernel {WC.wgrad_shape(d)}, meant for {kernel}"
    used = WC.wgrad_splits(d)
    assert used >= 1 and (splits == 0 or used <= splits)
    buf = Guarded(1, c.N * c.Ktot)
    buf.load(pre)
    d.dwp, d.splits = buf.ptr(), used
    assert launch(d, dtype) == 0, what
    got, untouched = buf.read()
    assert not bool(untouched.any())
    got = got.view(c.N, c.Ktot)
    assert torch.equal(got[mag == 0], pre.double()[mag == 0]), f"{what}: a structural zero changed the pre-loaded panel"
    check_panel(got, ref, mag, pre, coeff(c, used), dtype, f"{what} ({used} ranges)", kernel)
    return used


# ---------------------------------------------------------------------------------------------
# every case: slab mode with the library's own split plan, atomic mode onto a pre-load
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", [c.name for c in WC.PARITY_CASES])
def test_slabs_and_atomics_against_f64(name, dtype):
    run_slabs(name, dtype, f"{name} slabs")
    run_atomic(name, dtype, f"{name} atomic")


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_long_pixel_range_under_three_split_plans(dtype):
    """8192 pixels on the 256x256 kernel with the stand-alone plan, the plan of an overlapped launch and one explicit range: at
    least two of the three slab counts differ (else the plans are not told apart), all three meet the bound."""
    name = WC.P256_LONG.name
    used = [run_slabs(name, dtype, f"{name} automatic")[1], run_slabs(name, dtype, f"{name} overlapped", overlapped=1)[1],
            run_slabs(name, dtype, f"{name} splits = 1", splits=1)[1]]
    print(f"[parity] {name} {tag(dtype)}: slabs used: automatic {used[0]}, overlapped {used[1]}, explicit {used[2]}")
    assert used[2] == 1 and len(set(used)) >= 2, used


# ---------------------------------------------------------------------------------------------
# launch modes on one case per kernel
# ---------------------------------------------------------------------------------------------
MODES = ["atomic-3", "splits-1", "splits-3", "splits-beyond-stages", "slab-gap", "accumulate"]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", sorted(WC.MODE_CASES))
def test_launch_modes(kernel, mode, dtype):
    name = WC.MODE_CASES[kernel]
    c = WC.case(name)
    stages = -(-c.M // 64)
    what = f"{name} {mode}"
    if mode == "atomic-3":
        assert 2 <= run_atomic(name, dtype, what, splits=3) <= 3
    elif mode == "splits-1":
        assert run_slabs(name, dtype, what, splits=1)[1] == 1
    elif mode == "splits-3":
        assert 2 <= run_slabs(name, dtype, what, splits=3)[1] <= 3
    elif mode == "splits-beyond-stages":
        # more ranges than 64-pixel stages: the query answers a smaller count (run_slabs asserts that it is stable and that
        # exactly that many slabs are written)
        assert run_slabs(name, dtype, what, splits=stages + 5)[1] == stages
    elif mode == "slab-gap":
        run_slabs(name, dtype, what, splits=3, gap=100)
    else:
        # no kernel reads `accumulate` (header: reserved): slab mode stores either way, bit for bit the same
        a, _ = run_slabs(name, dtype, what + " = 0", splits=3, accumulate=0)
        b, _ = run_slabs(name, dtype, what + " = 1", splits=3, accumulate=1)
        assert torch.equal(a, b), f"{what}: the slabs depend on `accumulate`"


# ---------------------------------------------------------------------------------------------
# the ring kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", [c.name for c in WC.RING_CASES])
def test_ring_kernel_against_f64(name, dtype):
    """Slab mode with the slab count of the query; any other `splits` is UCLSTM_E_BADARG and writes nothing; with slab = 0 the
    same descriptor goes to another kernel, which is held to the same reference in atomic mode."""
    c, xd, dyd, _, _ = prepared(name, dtype)
    _, grid = run_slabs(name, dtype, f"{name} slabs")
    buf = Guarded(1, c.N * c.Ktot)
    for splits in sorted({0, 1, grid - 1, grid + 1} - {grid}):
        d = desc_of(c, xd, dyd, splits=splits, dwp=buf.ptr())
        assert WC.wgrad_shape(d) == 4
        assert launch(d, dtype) == E_BADARG, f"{name}: splits = {splits} accepted where the query says {grid}"
    assert bool(buf.read()[1].all()), f"{name}: a rejected launch wrote to dwp"
    assert c.atomic_shape in (0, 1, 2)
    run_atomic(name, dtype, f"{name} slab = 0", kernel=c.atomic_shape)


# ---------------------------------------------------------------------------------------------
# descriptors the library must refuse
# ---------------------------------------------------------------------------------------------
def test_rejected_descriptors():
    for what, d in WC.rejected_descriptors():
        assert WC.wgrad_splits(d) == E_BADARG, what
        assert WC.wgrad_shape(d) == E_BADARG, what


# ---------------------------------------------------------------------------------------------
# UCLSTM_WGRAD_GENERIC=1: power-of-two cases through the generic kernel (one child process; keep this test last)
# ---------------------------------------------------------------------------------------------
def child_main():
    for name in WC.FORCED_GENERIC:
        for dtype in DTYPES:
            run_slabs(name, dtype, f"{name} forced generic", kernel=0)
            run_atomic(name, dtype, f"{name} forced generic atomic", kernel=0)
    print_summary()


CHILD = "import sys; sys.path[:0] = sys.argv[1:3]; import test_gpu_wgrad_abi as T; T.child_main()"


def test_power_of_two_cases_through_the_generic_kernel():
    env = {k: v for k, v in os.environ.items() if not k.startswith("UCLSTM_WGRAD_")}
    env["UCLSTM_WGRAD_GENERIC"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT_DIR, os.path.join(ROOT_DIR, "tests")], env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout.replace("[parity-summary] wgrad kernel 0", "[parity-summary] wgrad kernel 0 (UCLSTM_WGRAD_GENERIC=1)"))
    assert r.returncode == 0, f"child failed ({r.returncode}): {r.stderr[-3000:]}"
    assert r.stdout.count("[parity] ") == 4 * len(WC.FORCED_GENERIC)
