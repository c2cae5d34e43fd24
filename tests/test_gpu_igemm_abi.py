"""The implicit-GEMM forward family (csrc/igemm_fwd.hip: per-tap 128x128 and 64x256, the patch loop in tile and strip mode, the
64 -> 64 ring kernel; STORE, fused ConvLSTM cell and split-K epilogues; 5x5 / 7x7; the group launch) called directly at the C ABI
with hand-built descriptors, in bf16 and fp16, and compared element by element with a host f64 reference that restates the
contract of include/uclstm.h (tests/igemm_cases.py; pinned to PyTorch's f64 convolutions by tests/test_cabi_and_host.py).

The reference multiplies the 16-bit activations that were uploaded with the panel read back from the device (filled by
ops.pack_weights, which has its own bit-exact test), so the only differences are f32 accumulation and the final rounding:
  * f32 outputs (slabs, atomics)    |err| <= c * mag,  c = max(2e-6, (Ktot/32 + ksplit + 2) * 2^-24): one f32 rounding per MFMA
                                    accumulation step (32 K elements each) plus one per atomic add; mag = sum_k |A * Wp| (+ |preload|)
  * 16-bit outputs                  |err| <= max(u16 * 1.01 * |ref|, floor) + 2^-21 * mag, u16 = half a unit in the last place
                                    (2^-8 bf16, 2^-11 fp16); floor = 2^-25 for fp16 (half its subnormal spacing: subnormal results
                                    are compared, not excluded), 0 for bf16.  After the affine, mag = (mag + |bias|) * |col_scale| +
                                    |col_shift|.  ReLU is 1-Lipschitz: nothing is re-drawn near the kink.
  * stats                           every [group][tile][n] slot against the f64 sum / sum of squares of the kernel's OWN stored
                                    16-bit values over that tile's pixels, at 2e-6 of sum|terms|; pad columns are never written
  * fused cell                      with dpre = c * mag and E = 2^-21 (the absolute error allowed to one fast_sigmoid / fast_tanh /
                                    f32 cell update): |di|, |df|, |do| <= dpre/4 + E, |dg| <= dpre + E, |dc| <= |c_prev| df + |g| di +
                                    |i| dg + E, h at half a 16-bit unit + do + dc + E, gates at half a unit + their f32 term.
                                    |c_prev| <= 2 in these cases, so the two f32 roundings of f*c + i*g (2^-23 * |c|) fit in E.
Every output buffer is pre-filled with a NaN bit pattern and sits between guard zones of the same pattern; an element the contract
does not write must still hold the pattern, every other element is compared, none is left out.

Pad hidden channels (Hd <= hc < Hd_p) of the fused cell are COMPUTED like any other channel, from zero panel rows: with zero bias /
pre_add / c_prev there (what pack_bias and the state tensors provide) c_out = h_out = 0 and the gates are exactly (0.5, 0.5, 0, 0.5).

The ring kernel's persistent blocks own more than one tile only above 256 tiles; case S13-e (259 tiles, 7 groups) reaches the merged
statistics rows: a block writes the sum of its consecutive tiles of one group into the last slot of that run and zeros into
the others, and three group boundaries fall inside a block's run.
"""
import ctypes as C
import functools

import pytest
import torch

import igemm_cases as IC
from igemm_cases import ALL_CASES, ATOMIC_CASES, LSTM_CASES, STORE_CASES

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_convlstm_amd import ops

L = IC.L
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
PATTERN = 0x7FE5                 # a NaN in bf16 and in fp16
GUARD = 4096                     # elements before and after every output buffer
E_ACT = 2.0 ** -21
WORST = {}                       # (what, dtype tag) -> worst |err| / bound, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """After the module's last test: the worst measured |err| / bound of every kernel / epilogue (the DESIGN.md table; run with -s)."""
    yield
    for (what, t), v in sorted(WORST.items()):
        print(f"[parity-summary] {what} {t}: {v:.3e}")


def tag(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


def u16(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def f32_coeff(c, ksplit=1):
    return max(2e-6, (c.Ktot / 32 + ksplit + 2) * 2.0 ** -24)


def note(what, dtype, worst):
    key = (what, tag(dtype))
    WORST[key] = max(WORST.get(key, 0.0), worst)


class Guarded:
    """A device buffer of `shape` between two guard zones, all filled with a NaN bit pattern."""

    def __init__(self, shape, dtype):
        self.n = 1
        for s in shape:
            self.n *= s
        self.shape, self.dtype = tuple(shape), dtype
        if dtype == torch.float32:
            self.pattern = 0x7FC00E50 | PATTERN
            self.raw = torch.full((self.n + 2 * GUARD,), self.pattern, dtype=torch.int32, device=DEV)
        else:
            self.pattern = PATTERN
            self.raw = torch.full((self.n + 2 * GUARD,), self.pattern, dtype=torch.int16, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.n].view(dtype).view(self.shape)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def load(self, x):
        self.t.copy_(x.to(self.dtype).view(self.shape))

    def read(self):
        """(values as f64 on the host, mask of elements that still hold the pattern); asserts the guards are intact."""
        raw = self.raw.cpu()
        assert bool((raw[:GUARD] == self.pattern).all()) and bool((raw[GUARD + self.n:] == self.pattern).all()), "write outside the buffer"
        body = raw[GUARD:GUARD + self.n]
        return body.view(self.dtype).view(self.shape).double(), (body == self.pattern).view(self.shape)


def check_16bit(got, untouched, ref, mag, dtype, what, key, f32_term=None):
    """Every element: the pattern where ref is NaN (nothing written), else |got - ref| <= max(u16*1.01*|ref|, floor) + f32 term."""
    skip = torch.isnan(ref)
    assert torch.equal(untouched, skip), f"{what}: {int((untouched != skip).sum())} elements written / left out against the contract"
    r, g = ref[~skip], got[~skip]
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite values stored"
    floor = 2.0 ** -25 if dtype == torch.float16 else 0.0
    term = (2.0 ** -21 * mag[~skip]) if f32_term is None else f32_term[~skip]
    bound = (u16(dtype) * 1.01 * r.abs()).clamp(min=floor) + term + 1e-30
    d = (g - r).abs()
    worst = float((d / bound).max()) if d.numel() else 0.0
    print(f"[parity] {what} {tag(dtype)}: worst |err| / bound {worst:.3f} (<= 1), max |err| {float(d.max()):.3e} over {d.numel()} elements")
    note(key, dtype, worst)
    bad = int((d > bound).sum())
    assert bad == 0, f"{what}: {bad} of {d.numel()} elements beyond the bound (worst {worst:.3f} x)"


def check_f32(got, ref, bound, dtype, what, key):
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: elements not written"
    d = (got - ref).abs()
    worst = float((d / (bound + 1e-30)).max())
    print(f"[parity] {what} {tag(dtype)}: worst |err| / bound {worst:.3f} (<= 1), max |err| {float(d.max()):.3e} over {d.numel()} elements")
    note(key, dtype, worst)
    bad = int((d > bound + 1e-30).sum())
    assert bad == 0, f"{what}: {bad} of {d.numel()} elements beyond the bound (worst {worst:.3f} x)"
    return d


def dev32(x):
    return x.float().to(DEV).contiguous()


def assert_shape(c, d):
    shp = int(L.lib.uclstm_igemm_fwd_shape(C.byref(d)))
    assert shp == c.shape, f"{c.name}: dispatches to kernel {shp}, the case is meant for {c.shape}"


def launch(d, dtype, what):
    L.check(L.kernels(dtype).uclstm_igemm_fwd(C.byref(d), ops._stream()), what)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=4)
def operands(name, dtype):
    """Activations (16-bit, host and device), the device panel and its host copy, and the f64 A operand of a case."""
    c = next(x for x in ALL_CASES + IC.GROUP_B if x.name == name)
    torch.manual_seed(1000 + sum(map(ord, name)))
    xs = [(torch.randn(c.n_img, Hs, Ws, Cs) * 0.8).to(dtype) for Cs, Hs, Ws, _, _ in c.srcs]
    xd = [x.to(DEV).contiguous() for x in xs]
    wshape = IC.weight_shape(c)
    fan = c.ktap * c.ktap * sum(s[0] for s in c.srcs)
    w = (torch.randn(wshape) * (1.6 / fan ** 0.5)).to(DEV)
    wp = ops.pack_weights(IC.pack_desc(c), w, dtype=dtype)
    assert tuple(wp.shape) == (c.N, c.Ktot)
    wph = wp.cpu()
    assert float((wph.float() != 0).float().mean()) > 0.02
    A = IC.gather_a(c.n_img, c.H, c.W, c.ktap, c.scale, c.pad, [(x, s[3], s[4]) for x, s in zip(xs, c.srcs)])
    return c, xd, wp, wph, A


# ---------------------------------------------------------------------------------------------
# STORE epilogue
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", [c.name for c in STORE_CASES])
def test_store_epilogue_against_f64(name, dtype):
    """Every STORE case of the table: bias / affine / ReLU, segments with scale, offset and c_off, dropped pixels, and `stats` slot
    by slot."""
    c, xd, wp, wph, A = operands(name, dtype)
    ref, mag = IC.gemm_ref(A, wph)
    bias = col_scale = col_shift = None
    if c.bias:
        bias = torch.randn(c.N) * 0.5
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if c.affine:
        col_scale = (torch.rand(c.N) + 0.5) * torch.where(torch.arange(c.N) % 3 == 0, -1.0, 1.0)
        col_shift = torch.randn(c.N) * 0.5
        ref = ref * col_scale.double() + col_shift.double()
        mag = mag * col_scale.double().abs() + col_shift.double().abs()
    if c.relu:
        ref = ref.clamp(min=0.0)
    segs = c.segments()
    outs = [Guarded((c.n_img, s[4], s[5], s[2]), dtype) for s in segs]
    tiles = IC.stats_tiles(c) if c.stats else None
    stats = Guarded((len(tiles), c.N, 2), torch.float32) if c.stats else None
    if c.stats:
        assert len(tiles) == c.groups * int(L.lib.uclstm_igemm_tiles_per_group(c.n_img, c.H, c.W, c.groups, c.N))
    keep = [dev32(t) if t is not None else None for t in (bias, col_scale, col_shift)]
    d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), [o.ptr() for o in outs],
                      *[None if t is None else t.data_ptr() for t in keep], stats.ptr() if stats else None)
    assert_shape(c, d)
    launch(d, dtype, name)
    refs, mags = IC.scatter_segments(ref, c.n_img, c.H, c.W, segs), IC.scatter_segments(mag, c.n_img, c.H, c.W, segs)
    for i, (o, s) in enumerate(zip(outs, segs)):
        got, untouched = o.read()
        check_16bit(got, untouched, refs[i], mags[i], dtype, f"{name} segment {i}", f"STORE kernel {c.shape}")
        assert int((~untouched).sum()) > 0
    if c.stats:
        # the stored values, GEMM-shaped (this needs the one-segment, output-grid cases the table uses for stats)
        assert len(segs) == 1 and segs[0][6:] == (1, 0, 0) and segs[0][3] == 0 and segs[0][0] == 0
        ncol = segs[0][1]
        stored = outs[0].read()[0].view(c.M, segs[0][2])[:, :ncol]
        sgot, suntouched = stats.read()
        assert not bool(suntouched.any()), f"{name}: statistics slots not written"
        runs = IC.stats_runs(c)
        for zeros, _, _ in runs:
            assert bool((sgot[zeros] == 0).all()), f"{name}: a slot inside a block's run is not zero"
        last = [r[1] for r in runs]
        sref = torch.stack([torch.stack((stored[p].sum(0), (stored[p] ** 2).sum(0)), -1) for _, _, p in runs])
        sabs = torch.stack([torch.stack((stored[p].abs().sum(0), (stored[p] ** 2).sum(0)), -1) for _, _, p in runs])
        e = float(((sgot[last, :ncol] - sref).abs() / (sabs + 1e-30)).max())
        print(f"[parity] {name} stats {tag(dtype)}: max |err| / sum|terms| {e:.2e} (<= 2e-6) over {sref.numel()} sums, "
              f"{sum(len(r[0]) for r in runs)} zero slots")
        note(f"stats kernel {c.shape}", dtype, e / 2e-6)
        assert e <= 2e-6, f"{name}: statistics slot off by {e:.3e} of sum|terms|"
        if ncol < c.N:
            # columns the segment does not store (ring kernel, n_end < N): the kernel sums the values it rounded but did not
            # write.  They cannot be read back, so they are held to the f64 values: each within its element bound b, hence
            # |sum - sum ref| <= sum b and |sumsq - sum ref^2| <= sum (2 |ref| b + b^2), plus 2e-6 of sum|terms| for the summation
            r, m = ref[:, ncol:], mag[:, ncol:]
            b = (u16(dtype) * 1.01 * r.abs()).clamp(min=2.0 ** -25 if dtype == torch.float16 else 0.0) + 2.0 ** -21 * m
            xref = torch.stack([torch.stack((r[p].sum(0), (r[p] ** 2).sum(0)), -1) for _, _, p in runs])
            xbnd = torch.stack([torch.stack((b[p].sum(0) + 2e-6 * r[p].abs().sum(0),
                                             (2 * r[p].abs() * b[p] + b[p] ** 2).sum(0) + 2e-6 * (r[p] ** 2).sum(0)), -1) for _, _, p in runs])
            check_f32(sgot[last, ncol:], xref, xbnd, dtype, f"{name} stats of the unstored columns", f"stats of unstored columns kernel {c.shape}")


# ---------------------------------------------------------------------------------------------
# split-K: slabs and atomics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", [c.name for c in ATOMIC_CASES])
def test_split_k_slabs_and_atomics_against_f64(name, dtype):
    """Slab mode: acc_ld = N + 8, one slab more than requested; each used slab equals the f64 partial sum over its own K range,
    the extra columns and the slabs beyond ksplit_used keep the NaN pattern.  Atomic mode: preload + full sum."""
    c, xd, wp, wph, A = operands(name, dtype)
    used = int(L.lib.uclstm_igemm_ksplit_used(c.Ktot, c.ktap, c.ksplit))
    assert used == IC.ATOMIC_USED[name.split("-")[-1]]
    masks = IC.krange_masks(c.ktap, c.ksegs, c.ksplit)
    assert len(masks) == used and int(torch.stack(masks).sum()) == c.Ktot
    ld = c.N + 8
    slabs = Guarded((c.ksplit + 1, c.M, ld), torch.float32)
    d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), acc_out=slabs.ptr(), acc_ld=ld, acc_slab=c.M * ld)
    assert_shape(c, d)
    launch(d, dtype, name + " slabs")
    got, untouched = slabs.read()
    expect_untouched = torch.ones_like(untouched)
    expect_untouched[:used, :, :c.N] = False
    assert torch.equal(untouched, expect_untouched), f"{name}: slab elements written / left out against the contract"
    coeff = f32_coeff(c, c.ksplit)
    for r, km in enumerate(masks):
        ref, mag = IC.gemm_ref(A, wph, km)
        check_f32(got[r, :, :c.N], ref, coeff * mag, dtype, f"{name} slab {r}", f"split-K slabs kernel {c.shape}")
    # atomic mode on a pre-loaded accumulator
    pre = torch.randn(c.M, ld)
    acc = Guarded((c.M, ld), torch.float32)
    acc.load(pre)
    d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), acc_out=acc.ptr(), acc_ld=ld, acc_slab=0)
    assert_shape(c, d)
    launch(d, dtype, name + " atomic")
    got, untouched = acc.read()
    assert not bool(untouched.any())
    ref, mag = IC.gemm_ref(A, wph)
    check_f32(got[:, :c.N], ref + pre.double()[:, :c.N], (coeff + c.ksplit * 2.0 ** -24) * (mag + pre.double()[:, :c.N].abs()), dtype,
              f"{name} atomic", f"split-K atomics kernel {c.shape}")
    assert torch.equal(got[:, c.N:].float(), pre[:, c.N:]), "columns beyond N of the accumulator changed"


# ---------------------------------------------------------------------------------------------
# fused ConvLSTM cell
# ---------------------------------------------------------------------------------------------
def lstm_inputs(c):
    """bias [N], pre_add [M][N] (panel-row order) and c_prev [M][Hd_p], zero on pad hidden channels.  With pre_add: a quarter of
    the pixels gets a closed input gate (pre_i - 30) and a cell state of 1e-5 (c_out ~ 1e-5: the tanh form cancels), another
    quarter gates pushed to +-30 (saturation)."""
    torch.manual_seed(77 + sum(map(ord, c.name)))
    M, N, Hp, Hd = c.M, c.N, c.Hd_p, c.Hd
    live = (torch.arange(N // 4) < Hd).float()
    to_rows = lambda g: g.reshape(-1, 4, N // 64, 16).permute(0, 2, 1, 3).reshape(-1, N)
    bias = to_rows((torch.randn(1, 4, N // 4) * 0.3) * live)[0] if c.bias else None
    c_prev = None
    if "no_c_prev" not in c.opts:
        c_prev = (torch.randn(M, Hp).clamp(-2.0, 2.0)) * live[:Hp]
    pre_add = None
    if "pre_add" in c.opts:
        pa = torch.randn(M, 4, N // 4) * 0.5
        q = torch.arange(M) % 4
        pa[q == 1, 0] -= 30.0
        sat = torch.where(torch.rand(M, 4, N // 4) < 0.5, -30.0, 30.0)
        pa[q == 2] += sat[q == 2]
        pre_add = to_rows(pa * live)
        if c_prev is not None:
            c_prev[q == 1] *= 1e-5
    return bias, pre_add, c_prev


def run_lstm(c, dtype, xd, wp, bias, pre_add, c_prev, with_gates=True):
    M, Hp = c.M, c.Hd_p
    c_out, h_out = Guarded((M, Hp), torch.float32), Guarded((M, Hp), dtype)
    gates = Guarded((M, 4, Hp), dtype) if with_gates else None
    keep = [None if t is None else dev32(t) for t in (bias, pre_add, c_prev)]
    d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), bias=None if keep[0] is None else keep[0].data_ptr(),
                      pre_add=None if keep[1] is None else keep[1].data_ptr(), c_prev=None if keep[2] is None else keep[2].data_ptr(),
                      c_out=c_out.ptr(), h_out=h_out.ptr(), gates_out=gates.ptr() if gates else None)
    assert_shape(c, d)
    launch(d, dtype, c.name)
    return d, keep, c_out, h_out, gates


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", [c.name for c in LSTM_CASES])
def test_fused_lstm_epilogue_against_f64(name, dtype):
    """Gates, c_out and h_out of the fused cell against train/unet.py:29-35 in f64 on pre = gemm + pre_add + bias; a second launch
    without gates_out gives bit-identical h_out / c_out.  Pad hidden channels: see the module docstring."""
    c, xd, wp, wph, A = operands(name, dtype)
    bias, pre_add, c_prev = lstm_inputs(c)
    _, _, c_out, h_out, gates = run_lstm(c, dtype, xd, wp, bias, pre_add, c_prev)
    pre, mag = IC.gemm_ref(A, wph)
    for t in (bias, pre_add):
        if t is not None:
            pre, mag = pre + t.double(), mag + t.double().abs()
    Hp = c.Hd_p
    pre, mag = IC.lstm_rows_to_gates(pre, Hp), IC.lstm_rows_to_gates(mag, Hp)
    cp = torch.zeros(c.M, Hp, dtype=torch.float64) if c_prev is None else c_prev.double()
    gref, cref, href = IC.lstm_cell_ref(pre, cp)
    dpre = f32_coeff(c) * mag
    dg = torch.stack((dpre[:, 0] / 4, dpre[:, 1] / 4, dpre[:, 2], dpre[:, 3] / 4), 1) + E_ACT
    dc = cp.abs() * dg[:, 1] + gref[:, 2].abs() * dg[:, 0] + gref[:, 0].abs() * dg[:, 2] + E_ACT
    cgot, cun = c_out.read()
    hgot, hun = h_out.read()
    ggot, gun = gates.read()
    assert not bool(cun.any()) and not bool(hun.any()) and not bool(gun.any()), f"{name}: elements not written"
    d = check_f32(cgot, cref, dc, dtype, f"{name} c_out", f"LSTM c_out kernel {c.shape}")
    print(f"[parity] {name} {tag(dtype)}: worst raw |c_out - c_ref| {float(d.max()):.3e}; where |c_ref| < 1e-4: "
          f"{float(d[cref.abs() < 1e-4].max()) if bool((cref.abs() < 1e-4).any()) else 0.0:.3e}")
    note("LSTM raw |c_out - c_ref|", dtype, float(d.max()))
    check_16bit(hgot, hun, href, None, dtype, f"{name} h_out", f"LSTM h_out kernel {c.shape}", f32_term=dg[:, 3] + dc + E_ACT)
    check_16bit(ggot, gun, gref, None, dtype, f"{name} gates", f"LSTM gates kernel {c.shape}", f32_term=dg)
    if "pre_add" in c.opts:
        assert float(pre.abs().max()) > 25.0 and bool((cref[:, :c.Hd].abs() < 1e-4).any()), "the saturated / tiny-state inputs are missing"
    if c.Hd < Hp:       # pad hidden channels: computed from zero rows
        assert bool((cgot[:, c.Hd:] == 0).all()) and bool((hgot[:, c.Hd:] == 0).all())
        assert bool((ggot[:, :, c.Hd:] == torch.tensor([0.5, 0.5, 0.0, 0.5], dtype=torch.float64)[None, :, None]).all())
    # inference form: no gates_out
    _, _, c2, h2, _ = run_lstm(c, dtype, xd, wp, bias, pre_add, c_prev, with_gates=False)
    assert torch.equal(c2.read()[0], cgot) and torch.equal(h2.read()[0], hgot), "h_out / c_out change when gates_out is NULL"


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", ["L0-hd64", "L2-tile"])
def test_activation_error_of_the_fused_cell_in_isolation(name, dtype):
    """fast_sigmoid and fast_tanh alone, through the f32 c_out: the panel is all zeros, so the GEMM is exactly 0 and every
    pre-activation is the f32 pre_add.  Half of the elements have a closed input gate (pre_i = -40) and c_prev = 1: c_out = sigmoid(v).
    The others have pre_i = +40 (i = 1.0f), pre_f = -40 and c_prev = 0: c_out = tanh(v).  v sweeps [-30, 30], +-1e-6 .. 1 and a
    normal draw.  Both must stay within E = 2^-21 of f64 (the allowance the cell bounds above give one activation)."""
    c, xd, _, _, _ = operands(name, dtype)
    torch.manual_seed(5)
    M, Hp, N = c.M, c.Hd_p, c.N
    n = M * Hp
    small = torch.logspace(-6, 0, n // 8)
    v = torch.cat((torch.linspace(-30, 30, n // 4), small, -small, torch.randn(n - n // 4 - 2 * (n // 8)) * 3))[torch.randperm(n)].view(M, Hp)
    kind = (torch.arange(n).view(M, Hp) % 2).bool()                 # False: sigmoid probe, True: tanh probe
    pa = torch.zeros(M, 4, N // 4)
    pa[:, 0, :Hp] = torch.where(kind, 40.0, -40.0)
    pa[:, 1, :Hp] = torch.where(kind, torch.tensor(-40.0), v)
    pa[:, 2, :Hp] = torch.where(kind, v, torch.tensor(0.0))
    pa[:, 3, :Hp] = v
    pre_add = pa.reshape(M, 4, N // 64, 16).permute(0, 2, 1, 3).reshape(M, N)
    c_prev = torch.where(kind, 0.0, 1.0)
    zero_panel = torch.zeros((c.N, c.Ktot), dtype=dtype, device=DEV)
    _, _, c_out, h_out, gates = run_lstm(c, dtype, xd, zero_panel, None, pre_add, c_prev)
    gref, cref, href = IC.lstm_cell_ref(IC.lstm_rows_to_gates(pre_add.double(), Hp), c_prev.double())
    cgot, cun = c_out.read()
    assert not bool(cun.any()) and bool(torch.isfinite(cgot).all())
    err = (cgot - cref).abs()
    e_sig, e_tanh = float(err[~kind].max()), float(err[kind].max())
    tiny = kind & (v.abs() < 1e-3)
    print(f"[parity] {name} {tag(dtype)}: activation error against f64 over {n} values: fast_sigmoid {e_sig:.3e}, fast_tanh {e_tanh:.3e} "
          f"(E = {E_ACT:.3e}); fast_tanh at |v| < 1e-3: {float(err[tiny].max()):.3e} absolute")
    note("E fast_sigmoid (absolute)", dtype, e_sig)
    note("E fast_tanh (absolute)", dtype, e_tanh)
    assert e_sig <= E_ACT and e_tanh <= E_ACT, f"activation error beyond 2^-21: sigmoid {e_sig:.3e}, tanh {e_tanh:.3e}"
    zero = torch.zeros_like(cref)
    check_16bit(gates.read()[0], gates.read()[1], gref, None, dtype, f"{name} gates (zero panel)", f"LSTM gates kernel {c.shape}", f32_term=torch.full_like(gref, E_ACT))
    check_16bit(h_out.read()[0], h_out.read()[1], href, None, dtype, f"{name} h_out (zero panel)", f"LSTM h_out kernel {c.shape}", f32_term=zero + 3 * E_ACT)


# ---------------------------------------------------------------------------------------------
# group launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("members", [IC.GROUP_A, IC.GROUP_B], ids=["three", "four"])
def test_group_launch_is_bit_identical_to_single_launches(members, dtype):
    """uclstm_igemm_fwd_group over unlike members (fused cells on tile and strip tiles, split-K slabs) against one launch each,
    and uclstm_igemm_fwd_group_blocks against the sum of the members' rounded grids."""
    singles, grouped, descs, keep = [], [], [], []
    for rnd in range(2):
        for c in members:
            _, xd, wp, _, _ = operands(c.name, dtype)
            if c.epi == L.EPI_LSTM:
                bias, pre_add, c_prev = lstm_inputs(c)
                M, Hp = c.M, c.Hd_p
                bufs = [Guarded((M, Hp), torch.float32), Guarded((M, Hp), dtype), Guarded((M, 4, Hp), dtype)]
                k = [None if t is None else dev32(t) for t in (bias, pre_add, c_prev)]
                p = [None if t is None else t.data_ptr() for t in k]
                d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), bias=p[0], pre_add=p[1], c_prev=p[2],
                                  c_out=bufs[0].ptr(), h_out=bufs[1].ptr(), gates_out=bufs[2].ptr())
            else:
                used = int(L.lib.uclstm_igemm_ksplit_used(c.Ktot, c.ktap, c.ksplit))
                bufs, k = [Guarded((used, c.M, c.N), torch.float32)], []
                d = IC.build_desc(c, [x.data_ptr() for x in xd], wp.data_ptr(), acc_out=bufs[0].ptr(), acc_ld=c.N, acc_slab=c.M * c.N)
            assert_shape(c, d)
            keep.append((xd, wp, k))
            if rnd == 0:
                launch(d, dtype, c.name)
                singles.append(bufs)
            else:
                descs.append(d)
                grouped.append(bufs)
    arr = (L.IgemmDesc * len(descs))(*descs)
    assert int(L.lib.uclstm_igemm_fwd_group_blocks(arr, len(descs))) == IC.group_blocks_expected(members)
    L.check(L.kernels(dtype).uclstm_igemm_fwd_group(arr, len(descs), ops._stream()), "igemm_fwd_group")
    torch.cuda.synchronize()
    for c, a, b in zip(members, singles, grouped):
        for x, y in zip(a, b):
            (vx, ux), (vy, uy) = x.read(), y.read()
            assert not bool(ux.any()) and not bool(uy.any()), f"{c.name}: elements not written"
            assert torch.equal(vx, vy), f"{c.name}: the group launch differs from the single launch"
