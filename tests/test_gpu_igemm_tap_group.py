"""uclstm_igemm_fwd_group_tap at the C ABI: up to four independent 3x3 descriptors of the 128 x 128 per-tap shape as ONE launch.

The contract (include/uclstm.h) is bit-identity with one uclstm_igemm_fwd launch per member, on every output buffer: h, c, gates
of a fused cell, every slab of a split-K member.  Outputs sit between guard zones filled with a NaN pattern and are compared as raw
bits, guards included, so a write outside a buffer or an element left unwritten in only one of the two runs fails too.  Anything
the entry point must refuse returns UCLSTM_E_BADARG from the launch AND from the validation-only twin and leaves the outputs
untouched.

Shapes: the smallest that exercise each path -- a 2 x 2 image (4 pixels: one partial tile, taps falling on padding all round), 3 x 9
x 11 (297 pixels: three tiles, the last partial; Hd = 24 pads the panel to 128 rows), split-K slabs with 2 and 3 used ranges, a
one-source cell with pre_add -- in groups of 1, 3 and 4 members with unlike K lengths, one of them listed shortest first."""
import ctypes as C
import dataclasses

import pytest
import torch

import igemm_cases as IC
from igemm_cases import Case, _lstm
from unet_convlstm_amd import ops

pytestmark = pytest.mark.gpu

L = IC.L
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 1024
BADARG = -1

A01 = [(72, 9, 11, 0, 0), (24, 9, 11, 0, 0)]          # 128 + 64 channels: three K chunks
CASES = {c.name: c for c in [
    _lstm("T-tiny", 0, 1, 2, 2, 24, 64, ("pre_add",)),                      # 4 pixels, 18 K-steps
    _lstm("T-odd", 0, 3, 9, 11, 24, 24, ("pre_add",)),                      # 297 pixels, Hd_p = 24 of 32 panel columns, 18 K-steps
    _lstm("T-long", 0, 2, 5, 7, 136, 64, ()),                               # 70 pixels, 192 + 64 channels: 36 K-steps
    _lstm("T-no-c-prev", 0, 1, 3, 5, 24, 40, ("no_c_prev", "no_bias")),
    Case("T-slab2", 0, 3, 9, 11, A01, 136, epi=L.EPI_ATOMIC, ksplit=2, bias=False),       # 2 ranges of 18 K-steps, N = 136: two row tiles
    Case("T-slab8", 0, 3, 9, 11, A01, 136, epi=L.EPI_ATOMIC, ksplit=8, bias=False),       # 8 asked, 3 used: 9 K-steps each
    _lstm("T1-h-only", 0, 3, 9, 11, 24, 21, ("pre_add",), single=True),
    Case("T1-slab2", 0, 2, 5, 7, [(72, 5, 7, 0, 0)], 136, epi=L.EPI_ATOMIC, ksplit=2, bias=False),
    # what the entry point must refuse
    _lstm("R-patch", 2, 1, 16, 16, 64, 64, ("pre_add",)),
    Case("R-shape1", 1, 3, 9, 11, A01, 40, epi=L.EPI_ATOMIC, ksplit=2, bias=False),
    dataclasses.replace(_lstm("R-5x5", 0, 1, 3, 5, 24, 40, ()), ktap=5, pad=2),
]}
GROUPS = {
    "one": ["T-tiny"],
    "three": ["T-odd", "T-slab2", "T-tiny"],
    "four-shortest-first": ["T-slab8", "T-long", "T-odd", "T-no-c-prev"],          # K-steps per block 9, 36, 18, 18
    "four": ["T-long", "T-slab2", "T-tiny", "T-slab8"],
    "one-source": ["T1-h-only", "T1-slab2"],
}


def tag(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp16"


class Guarded:
    """A device buffer between two guard zones, everything filled with a NaN bit pattern; compared as raw bits."""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        wide = dtype == torch.float32
        self.pattern = 0x7FC07FE5 if wide else 0x7FE5
        self.raw = torch.full((n + 2 * GUARD,), self.pattern, dtype=torch.int32 if wide else torch.int16, device=DEV)
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(tuple(shape))
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def untouched(self):
        return bool((self.raw == self.pattern).all())

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.pattern).all()) and bool((self.raw[-GUARD:] == self.pattern).all())

    def all_written(self):
        return not bool((self.raw[GUARD:-GUARD] == self.pattern).any())


def member(name, dtype, slab=True):
    """(case, descriptor, output buffers, tensors to keep alive) with fresh sentinel-filled outputs; inputs are a function of
    the case name, so two calls describe the same launch."""
    c = CASES[name]
    torch.manual_seed(500 + sum(map(ord, name)))
    xd = [(torch.randn(c.n_img, Hs, Ws, Cs) * 0.8).to(dtype).to(DEV).contiguous() for Cs, Hs, Ws, _, _ in c.srcs]
    fan = c.ktap * c.ktap * sum(s[0] for s in c.srcs)
    w = (torch.randn(IC.weight_shape(c)) * (1.6 / fan ** 0.5)).to(DEV)
    wp = ops.pack_weights(IC.pack_desc(c), w, dtype=dtype)
    assert tuple(wp.shape) == (c.N, c.Ktot)
    src = [x.data_ptr() for x in xd]
    if c.epi == L.EPI_LSTM:
        M, Hp = c.M, c.Hd_p
        bias = (torch.randn(c.N) * 0.3).to(DEV) if c.bias else None
        pre_add = (torch.randn(M, c.N) * 0.5).to(DEV) if "pre_add" in c.opts else None
        c_prev = None if "no_c_prev" in c.opts else torch.randn(M, Hp).clamp(-2, 2).to(DEV)
        bufs = [Guarded((M, Hp), torch.float32), Guarded((M, Hp), dtype), Guarded((M, 4, Hp), dtype)]
        p = [None if t is None else t.data_ptr() for t in (bias, pre_add, c_prev)]
        d = IC.build_desc(c, src, wp.data_ptr(), bias=p[0], pre_add=p[1], c_prev=p[2], c_out=bufs[0].ptr(), h_out=bufs[1].ptr(),
                          gates_out=bufs[2].ptr())
        keep = (xd, wp, bias, pre_add, c_prev)
    else:
        used = int(L.lib.uclstm_igemm_ksplit_used(c.Ktot, c.ktap, c.ksplit))
        bufs = [Guarded((used, c.M, c.N), torch.float32)]
        d = IC.build_desc(c, src, wp.data_ptr(), acc_out=bufs[0].ptr(), acc_ld=c.N, acc_slab=c.M * c.N if slab else 0)
        keep = (xd, wp)
    return c, d, bufs, keep


def blocks_expected(cases):
    """Sum of the members' own grids (128 x 128 tiles x used K ranges), each rounded up to a multiple of 8."""
    total = 0
    for c in cases:
        grid = -(-c.M // 128) * -(-c.N // 128)
        if c.epi == L.EPI_ATOMIC:
            grid *= int(L.lib.uclstm_igemm_ksplit_used(c.Ktot, c.ktap, c.ksplit))
        total += IC.roundup(grid, 8)
    return total


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("group", list(GROUPS))
def test_tap_group_launch_is_bit_identical_to_single_launches(group, dtype):
    K = L.kernels(dtype)
    singles = [member(name, dtype) for name in GROUPS[group]]
    for c, d, _, _ in singles:
        assert int(L.lib.uclstm_igemm_fwd_shape(C.byref(d))) == 0, c.name
        L.check(K.uclstm_igemm_fwd(C.byref(d), ops._stream()), c.name)
    grouped = [member(name, dtype) for name in GROUPS[group]]
    arr = (L.IgemmDesc * len(grouped))(*[m[1] for m in grouped])
    for i in range(len(grouped)):
        assert int(L.lib.uclstm_igemm_fwd_shape(C.byref(arr[i]))) == 0
    assert int(L.lib.uclstm_igemm_fwd_group_tap_blocks(arr, len(grouped))) == blocks_expected([m[0] for m in grouped])
    L.check(K.uclstm_igemm_fwd_group_tap(arr, len(grouped), ops._stream()), "igemm_fwd_group_tap")
    torch.cuda.synchronize()
    for (c, _, a, _), (_, _, b, _) in zip(singles, grouped):
        for what, x, y in zip(("c", "h", "gates") if c.epi == L.EPI_LSTM else ("slabs",), a, b):
            assert x.guards_intact() and y.guards_intact(), f"{c.name} {what}: write outside the buffer"
            assert x.all_written() and y.all_written(), f"{c.name} {what}: elements not written"
            assert torch.equal(x.raw, y.raw), f"{c.name} {what}: the group launch differs from the single launch"


def test_members_are_ordered_by_k_steps_per_block():
    """The case the order test relies on: the listed order of 'four-shortest-first' is not the longest-first order."""
    steps = []
    for name in GROUPS["four-shortest-first"]:
        c = CASES[name]
        chunks = sum(c.ksegs) // 64
        per = -(-chunks // c.ksplit) if c.epi == L.EPI_ATOMIC else chunks
        steps.append(9 * per)
    assert steps == [9, 36, 18, 18] and steps != sorted(steps, reverse=True)


REFUSALS = {
    "patch-shape member": (["T-odd", "R-patch"], 2, True),
    "shape-1 member": (["T-slab2", "R-shape1"], 2, True),
    "5x5 cell": (["R-5x5"], 1, True),
    "5x5 cell in a group": (["T-tiny", "R-5x5", "T-odd"], 3, True),
    "mixed nsrc": (["T-odd", "T1-h-only"], 2, True),
    "atomic accumulation": (["T-slab2"], 1, False),
    "n = 5": (["T-tiny", "T-odd", "T-slab2", "T-slab8", "T-long"], 5, True),
    "n = 0": (["T-tiny"], 0, True),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_return_badarg_and_launch_nothing(what, dtype):
    names, n, slab = REFUSALS[what]
    ms = [member(name, dtype, slab) for name in names]
    for c, d, _, _ in ms:           # every member is a valid descriptor of its own: it is the GROUP that is refused
        assert int(L.lib.uclstm_igemm_fwd_shape(C.byref(d))) == c.shape, c.name
    arr = (L.IgemmDesc * len(ms))(*[m[1] for m in ms])
    assert int(L.lib.uclstm_igemm_fwd_group_tap_blocks(arr, n)) == BADARG
    assert int(L.kernels(dtype).uclstm_igemm_fwd_group_tap(arr, n, ops._stream())) == BADARG
    torch.cuda.synchronize()
    for c, _, bufs, _ in ms:
        assert all(b.untouched() for b in bufs), f"{c.name}: a refused group wrote to an output"


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_patch_group_entry_still_refuses_per_tap_members(dtype):
    """uclstm_igemm_fwd_group keeps its contract: patch members only."""
    ms = [member(name, dtype) for name in ("T-odd", "T-tiny")]
    arr = (L.IgemmDesc * 2)(*[m[1] for m in ms])
    assert int(L.lib.uclstm_igemm_fwd_group_blocks(arr, 2)) == BADARG
    assert int(L.kernels(dtype).uclstm_igemm_fwd_group(arr, 2, ops._stream())) == BADARG
    torch.cuda.synchronize()
    assert all(b.untouched() for _, _, bufs, _ in ms for b in bufs)
