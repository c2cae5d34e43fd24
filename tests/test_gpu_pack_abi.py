"""The weight-panel kernels of csrc/pack.hip (pack, batched pack, unpack, ordered unpack, bias) and uclstm_splitk_finish, each
called directly at the C ABI -- bf16 and fp16 wherever the entry point has a twin -- and compared with the references of
tests/pack_cases.py, which restate include/uclstm.h; tests/test_pack_cases_host.py pins the descriptor builders behind them to
PyTorch's f64 convolutions and autograd.

Every weight and every weight gradient passes through these kernels on every step, but the GEMM parity tests build their panels on
the host.  The case table holds the smallest shapes that reach each path: the 256-channel chunk boundary of the row family, pad
rows inside a 16-row gate block, half-empty 16-row blocks and padding gate columns of the transposed family, the 4-tap
transposed kernel (family 4, no panel of the model uses it), 25- and 49-tap generic panels, the second trip of the generic
grid-stride loop; every residue of the three-slab loop of the row-family unpack, exact eights and tails of the fold kernel, the
64 / 65 threshold, the fold's alignment preconditions failing one at a time, the atomic split with an empty trailing group.
Every case asserts the kernel family (uclstm_pack_job_init) or path (preconditions restated in pack_cases.unpack_path) it was
written for.

Bounds -- counted, none measured:
  * pack, bias: bit-exact.  Weights hold signed zeros, infinities, NaN (compared as "NaN at the same positions"), half-way points
    of both parities, 65520, the largest finite f32, f32 and 16-bit subnormals.  Panels sit in a larger buffer pre-filled with a
    sentinel: padding is the +0 bit pattern, guards are unchanged.
  * unpack, one slab: bit-exact ((accumulate ? base : 0) + v is one f32 addition of the same operands on the CPU).
  * unpack, several slabs: |err| <= (nslab + 2) * 2^-24 * (sum|slab terms| + |base|): nslab - 1 additions of slabs, one of the
    base, in any order (covers the atomic split), each rounding at most 2^-24 of the magnitude.  With accumulate = 0 the mapped
    elements of grad start as NaN; elements the map does not reach keep their bits.
  * ordered unpack: bit-identical to the f32 host loop in the association the header states.
  * split-K finish: check_elementwise with f32_units = (nslab + 3) * 2^-24: nslab - 1 slab additions, the bias add, the multiply
    and the shift add, + half a 16-bit unit of the result.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_cases as PC
from test_gpu_boundary_abi import assert_bits, bits, check_f32
from test_gpu_pointwise_abi import DEV, DTYPES, call, check_elementwise, nan_like, tag

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops
    L = U._lib

GUARD = 64                                  # guard elements on either side of an output
F32_GUARD = 1234.5
F32_UNIT = 2.0 ** -24


def vp(t, byte_off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_off)


def guarded16(n, dtype):
    """(whole buffer, the n elements between the guards), every element the 0x5A5A sentinel."""
    buf = torch.full((n + 2 * GUARD,), PC.SENTINEL, dtype=torch.int16, device=DEV).view(dtype)
    return buf, buf[GUARD:GUARD + n]


def guarded32(body):
    """(whole f32 buffer, the view holding `body`) with F32_GUARD on either side."""
    buf = torch.full((body.numel() + 2 * GUARD,), F32_GUARD, dtype=torch.float32)
    buf[GUARD:GUARD + body.numel()] = body.reshape(-1)
    buf = buf.to(DEV)
    return buf, buf[GUARD:GUARD + body.numel()]


def assert_guards(buf, what):
    b = bits(buf)
    want = PC.SENTINEL if buf.element_size() == 2 else int(torch.tensor(F32_GUARD).view(torch.int32))
    assert bool((b[:GUARD] == want).all()) and bool((b[-GUARD:] == want).all()), f"{what}: guard elements were written"


def family_of(d):
    job = L.PackJob()
    return int(L.lib.uclstm_pack_job_init(C.byref(job), C.byref(d), 1 << 20, 1 << 20, 0))


def assert_panel(got, case, d, w, dtype, what):
    """got [N][Ktot] == pack_ref bit for bit: NaN at the same positions, every other element the same bits, padding +0."""
    ref = PC.pack_ref(d, w, case.elem_off, dtype)
    got = got.detach().cpu().view(d.N, d.Ktot)
    gn, rn = got.isnan(), ref.isnan()
    assert torch.equal(gn, rn), f"{what}: NaN at {int(gn.sum())} positions, the reference has {int(rn.sum())}"
    zero = torch.zeros((), dtype=dtype)
    assert_bits(torch.where(gn, zero, got), torch.where(rn, zero, ref), f"{what} ({int(rn.sum())} NaN, {int(ref.isinf().sum())} inf)")
    valid, _ = PC.index_map(d)
    assert bool((bits(got)[torch.from_numpy(~valid)] == 0).all()), f"{what}: padding is not +0"


# ---------------------------------------------------------------------------------------------
# 1. uclstm_pack_weights / uclstm_pack_weights_batched
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
def test_pack_weights_bit_exact(case, dtype):
    d = case.desc
    assert family_of(d) == case.family
    w = PC.weight_with_specials(case, dtype)
    wd = w.to(DEV)
    buf, panel = guarded16(d.N * d.Ktot, dtype)
    call(L.kernels(dtype), "uclstm_pack_weights", C.byref(d), vp(wd, 4 * case.elem_off), vp(panel))
    what = f"pack_weights {case.name} {tag(dtype)} [family {case.family}]"
    assert_panel(panel, case, d, w, dtype, what)
    assert_guards(buf, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_batched_packing_bit_exact_over_all_families(dtype):
    """uclstm_pack_weights_batched through ops._PackBatch (job table on the device, one launch per family and segment) over every
    case of the table, family 4 included, against pack_ref."""
    items, ws = [], []
    for case in PC.CASES:
        d = case.desc
        w = PC.weight_with_specials(case, dtype)
        wd = w.to(DEV)
        ws.append(w)
        items.append(((wd.data_ptr(), case.elem_off, bytes(d), dtype), d, wd, case.elem_off))
    assert len({it[0] for it in items}) == len(items)
    batch = ops._PackBatch(items)
    fams = sorted({f for launches in batch.segments for _, f, _, _, _ in launches})
    assert fams == [0, 1, 2, 3, 4] and len(batch.segments) > 1, fams
    for wp, _ in batch.panels.values():
        wp.view(torch.int16).fill_(PC.SENTINEL)
    batch.launch(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for (key, d, _, _), case, w in zip(items, PC.CASES, ws):
        assert_panel(batch.panels[key][0], case, d, w, dtype, f"pack_weights_batched {case.name} {tag(dtype)} [family {case.family}]")


# ---------------------------------------------------------------------------------------------
# 2. uclstm_unpack_wgrad
# ---------------------------------------------------------------------------------------------
ROWS_COUNTS = (1, 2, 3, 4, 6, 7, 64)              # all residues of the three-slab loop, and the last count of the row kernel
FOLD_COUNTS = (65, 66, 72, 73, 170)               # exact eights (1 + 8k) and tails of the fold kernel
GENERIC_COUNTS = (1, 5, 15, 16, 25, 300)
UNPACK_RUNS = (
    [(c.name, n, "plain") for c in PC.UNPACK_CASES if c.family != PC.FAM_GENERIC for n in ROWS_COUNTS + FOLD_COUNTS] +
    [("conv fwd c257", 70, v) for v in ("gap4", "gap1", "dwp+1")] +
    [(c.name, n, "plain") for c in PC.UNPACK_CASES if c.family == PC.FAM_GENERIC for n in GENERIC_COUNTS] +
    [("lstm h half hd5", n, "plain") for n in (3, 66)]                # a half descriptor into the full weight: unmapped elements
)
VARIANTS = {"plain": (0, 0), "gap4": (4, 0), "gap1": (1, 0), "dwp+1": (0, 1)}      # (floats between slabs beyond N*Ktot, dwp offset)


def slab_store(slabs, slab, shift):
    """Device buffer holding the slabs `slab` floats apart from element `shift` on, NaN in every gap: a fresh copy per call (the
    entry points consume dwp)."""
    nslab, total = slabs.shape
    store = torch.full((shift + nslab * slab + 4,), float("nan"))
    store[shift:shift + nslab * slab].view(nslab, slab)[:, :total] = slabs
    return store.to(DEV)


def unpack_inputs(case, nslab, seed):
    d = case.desc
    gen = torch.Generator().manual_seed(seed + nslab)
    slabs = torch.randn((nslab, d.N * d.Ktot), generator=gen)
    base = torch.randn(case.wshape, generator=gen)
    return d, slabs, base


@pytest.mark.parametrize("name,nslab,variant", UNPACK_RUNS, ids=lambda v: str(v))
def test_unpack_wgrad_against_f64(name, nslab, variant):
    """One slab: bit-exact.  Otherwise |err| <= (nslab + 2) * 2^-24 * (sum|slab terms| + |base|) (module docstring)."""
    case = PC.BY_NAME[name]
    d, slabs, base = unpack_inputs(case, nslab, 500)
    assert family_of(d) == case.family
    total = d.N * d.Ktot
    gap, shift = VARIANTS[variant]
    slab = total + gap
    want_path = {"plain": "generic" if case.family == PC.FAM_GENERIC else ("rows" if nslab <= 64 else "fold"),
                 "gap4": "fold", "gap1": "generic", "dwp+1": "generic"}[variant]
    for acc in (0, 1):
        sd = slab_store(slabs, slab, shift)
        assert sd.data_ptr() % 16 == 0
        assert PC.unpack_path(d, case.family, nslab, slab, sd.data_ptr() + 4 * shift) == want_path
        groups = PC.generic_groups(d, nslab) if (want_path == "generic" and acc) else 1
        if (name, nslab) == ("first layer ci1", 25) and acc:
            assert groups == 6 and 5 * 5 >= nslab                      # six groups of five slabs: group 5 is empty
        ref, mag, mapped = PC.unpack_ref(d, slabs.view(nslab, d.N, d.Ktot), base, acc)
        start = base.clone()
        if not acc:
            start.view(-1)[torch.from_numpy(mapped)] = float("nan")    # a kernel that reads grad with accumulate = 0 returns NaN
        gbuf, grad = guarded32(start)
        call(L.lib, "uclstm_unpack_wgrad", C.byref(d), vp(sd, 4 * shift), nslab, slab, vp(grad), acc)
        got = grad.cpu()
        what = f"unpack_wgrad {name} nslab={nslab} {variant} accumulate={acc} [{want_path}, {groups} groups]"
        assert_guards(gbuf, what)
        m = torch.from_numpy(mapped)
        assert bool(torch.isfinite(got[m]).all()), f"{what}: mapped elements not written, or grad was read with accumulate = 0"
        if not bool(m.all()):
            assert_bits(got[~m], base.view(-1)[~m], what + " unmapped elements")
        else:
            assert name != "lstm h half hd5"
        if nslab == 1:
            want, _ = PC.ordered_unpack_f32(d, slabs, base, acc)
            assert_bits(got, torch.from_numpy(want), what)
        else:
            got = torch.where(m, got, base.view(-1))
            check_f32(got, torch.from_numpy(ref), torch.from_numpy((nslab + 2) * F32_UNIT * mag), what)


# ---------------------------------------------------------------------------------------------
# 3. uclstm_unpack_wgrad_ordered
# ---------------------------------------------------------------------------------------------
ORDERED_RUNS = (
    [(n, k) for n in ("conv fwd c257", "conv fwd 264+24", "lstm wgrad hd5") for k in (1, 7, 64, 65, 170)] +
    # one generic descriptor per n-mode: IDENTITY, TAPMAJOR, LSTM (the last one has 800 blocks of elements: one group at any count)
    [(n, k) for n in ("first layer ci2", "convT fwd co20", "lstm 5x5") for k in (1, 7, 25, 300)]
)


@pytest.mark.parametrize("name,nslab", ORDERED_RUNS, ids=lambda v: str(v))
def test_unpack_wgrad_ordered_bit_identical_to_the_host_loop(name, nslab):
    """One group: t = s0; t += s1; ...; out = (accumulate ? base : 0) + t in f32, and the bits of uclstm_unpack_wgrad on the same
    input with accumulate = 0.  Several groups: the header's two stages, scratch rows included."""
    case = PC.BY_NAME[name]
    d, slabs, base = unpack_inputs(case, nslab, 900)
    total = d.N * d.Ktot
    G = int(L.lib.uclstm_unpack_wgrad_ordered_groups(C.byref(d), nslab))
    assert G == PC.ordered_groups(d, case.family, nslab)
    if case.family != PC.FAM_GENERIC:
        assert G == 1
    _, _, mapped = PC.unpack_ref(d, slabs.view(nslab, d.N, d.Ktot), base, 0)
    assert bool(mapped.all())
    for acc in (0, 1):
        start = base.clone() if acc else torch.full(case.wshape, float("nan"))
        gbuf, grad = guarded32(start)
        scratch = nan_like((G, total), torch.float32) if G > 1 else None
        sd = slab_store(slabs, total, 0)
        call(L.lib, "uclstm_unpack_wgrad_ordered", C.byref(d), vp(sd), nslab, total, vp(scratch), vp(grad), acc)
        what = f"unpack_wgrad_ordered {name} nslab={nslab} accumulate={acc} [{G} groups]"
        want, scr = PC.ordered_unpack_f32(d, slabs, base, acc, G)
        assert_guards(gbuf, what)
        assert_bits(grad.cpu(), torch.from_numpy(want), what)
        if G > 1:
            assert_bits(scratch.cpu(), torch.from_numpy(scr), what + " scratch")
        elif not acc:
            g2buf, g2 = guarded32(torch.full(case.wshape, float("nan")))
            sd = slab_store(slabs, total, 0)
            call(L.lib, "uclstm_unpack_wgrad", C.byref(d), vp(sd), nslab, total, vp(g2), 0)
            assert_bits(g2.cpu(), grad.cpu(), what + " == uclstm_unpack_wgrad")


# ---------------------------------------------------------------------------------------------
# 4. uclstm_pack_bias
# ---------------------------------------------------------------------------------------------
BIAS_CASES = {
    "identity N > n_valid": lambda: PC.conv_fwd(20, [24]),
    "lstm hd5": lambda: ops.lstm_pack_desc(5, 8),
    "lstm hd24": lambda: ops.lstm_pack_desc(24, 8),
    "lstm hd72": lambda: ops.lstm_pack_desc(72, 8),                  # N = 320: a second block
    "tap-major convT": lambda: ops.convt_pack_desc(48, 20),          # the bias repeated under each of the four taps
}


@pytest.mark.parametrize("name", list(BIAS_CASES))
def test_pack_bias_bit_exact(name):
    d = BIAS_CASES[name]()
    torch.manual_seed(1200 + d.N)
    b = torch.randn(PC.bias_len(d))
    b[1], b[2], b[-1] = -0.0, float("inf"), float("-inf")
    ref = PC.bias_ref(d, b)
    ok_n, _, _ = PC.row_map(d)
    assert d.N > int(ok_n.sum()) and (name != "lstm hd72" or d.N > 256)
    buf, bp = guarded32(torch.full((d.N,), float("nan")))
    bd = b.to(DEV)
    call(L.lib, "uclstm_pack_bias", C.byref(d), vp(bd), vp(bp))
    what = f"pack_bias {name} (N = {d.N})"
    assert_bits(bp.cpu(), ref, what)
    assert bool((bits(bp)[torch.from_numpy(~ok_n)] == 0).all()), f"{what}: padding rows are not +0"
    assert_guards(buf, what)


# ---------------------------------------------------------------------------------------------
# 5. uclstm_splitk_finish
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", PC.SPLITK_CASES, ids=str)
def test_splitk_finish_against_f64(case, dtype):
    """|err| <= half a 16-bit unit of the result + (nslab + 3) * 2^-24 * ((sum|slabs| + |bias|) * |scale| + |shift|): the kernel
    adds the slabs in order (nslab - 1 roundings), then (v + bias) * scale + shift (three, or two when contracted)."""
    pixels, Cc, ld, nslab, extra, relu, _ = case
    pre, body, bias, scale, shift = PC.splitk_input(case, dtype)
    slab = pixels * ld + extra
    ref, mag = PC.splitk_finish_ref(pre[:, :pixels * ld].view(nslab, pixels, ld), bias, scale, shift, relu, Cc)
    buf, out = guarded16(pixels * Cc, dtype)
    out.fill_(float("nan"))
    pd = pre.to(DEV)
    dv = [None if t is None else t.to(DEV) for t in (bias, scale, shift)]
    call(L.kernels(dtype), "uclstm_splitk_finish", vp(pd), nslab, slab, ld, vp(dv[0]), vp(dv[1]), vp(dv[2]), relu, vp(out), pixels, Cc)
    what = f"splitk_finish {case} {tag(dtype)}"
    check_elementwise(out.cpu().view(pixels, Cc), ref, mag, dtype, what, f32_units=(nslab + 3) * F32_UNIT)
    if relu:
        assert bool((out >= 0).all())
    assert_guards(buf, what)
