"""The GEMM families at the top of the 2 GiB range of their 32-bit buffer descriptors (tests/high_offset_cases.py; the table, the
boundaries and the selection rules are checked without a GPU by tests/test_high_offset_cases_host.py).

Every case launches its kernel at the C ABI with the largest image count the library admits, on operands generated on the
device between guard zones of a NaN bit pattern (a read that is off by a little multiplies a NaN), into outputs pre-filled with
that pattern.  Per-pixel kernels: every element of the sampled images against the f64 reference of igemm_cases, under the bounds
of tests/test_gpu_igemm_abi.py (its own check functions are called: no new tolerance); no element of the whole output may still
be NaN, the guards must be intact, and the statistics rows of the sampled BatchNorm groups are held to the kernel's own stored
values.  Group launches are compared bit for bit, whole buffers, with the single launches.  Weight gradients: dY is zero outside
the window images, so the full result is compared with the f64 sum over the windows under the bound of
tests/test_gpu_wgrad_abi.py, with the pixel count of the windows in place of M: a zero dY row adds exact zeros and no rounding
(the operands are multiples of 1/8, so a panel element is a sum of multiples of 1/64 far below 2^18: exact in f32, and slab mode
is also asserted to be EXACT, which one dropped pixel breaks).  Slab mode, atomic mode onto a pre-loaded panel and the unpack of
the slabs run once each.

The last tests go through ops with the real LAUNCH_BYTES_LIMIT: a tensor of exactly 2^31 bytes through igemm_store (image cuts
and whole-group cuts), through igemm_wgrad, and the hoisted x half of a ConvLSTM layer at the size where its loop cuts.

Run with -s for the worst |err| / bound of every case, the duration of every test and the peak device memory
(profiles/high_offset_parity.txt)."""
import ctypes as C
import dataclasses
import gc
import time

import pytest
import torch

import high_offset_cases as HC
import igemm_cases as IC
import test_gpu_igemm_abi as FA
import test_gpu_wgrad_abi as WA
import wgrad_cases as WC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from unet_convlstm_amd import ops

L = IC.L
DEV = "cuda"
GUARD = FA.GUARD
BF16, FP16 = torch.bfloat16, torch.float16
WORST = {}                       # (case, dtype tag) -> worst |err| / bound
TIMES = []                       # (test id, seconds)
tag = FA.tag


@pytest.fixture(scope="module", autouse=True)
def report():
    torch.cuda.reset_peak_memory_stats()
    yield
    for (what, t), v in sorted(WORST.items()):
        print(f"[high-offset-summary] {what} {t}: {v:.3e}")
    for what, s in TIMES:
        print(f"[high-offset-time] {what}: {s:.2f} s")
    print(f"[high-offset-memory] peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


@pytest.fixture(autouse=True)
def timed_and_freed(request):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    TIMES.append((request.node.name, time.perf_counter() - t0))
    gc.collect()
    torch.cuda.empty_cache()


def keep_worst(name, dtype, table, key):
    """Move what a check function of the ABI test files noted under `key` into this file's table."""
    v = table.pop((key, tag(dtype)))
    WORST[(name, tag(dtype))] = max(WORST.get((name, tag(dtype)), 0.0), v)


class Big:
    """A device buffer of `shape` between two guard zones, all filled with a NaN bit pattern; only what a test asks for is copied
    to the host."""

    def __init__(self, shape, dtype):
        self.n = 1
        for s in shape:
            self.n *= s
        wide = dtype == torch.float32
        self.pattern = 0x7FC07FE5 if wide else FA.PATTERN
        self.raw = torch.full((self.n + 2 * GUARD,), self.pattern, dtype=torch.int32 if wide else torch.int16, device=DEV)
        self.body = self.raw[GUARD:GUARD + self.n]
        self.t = self.body.view(dtype).view(tuple(shape))
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.pattern).all()) and bool((self.raw[GUARD + self.n:] == self.pattern).all())

    def pattern_left(self, step=1 << 28):
        """Number of elements that are NaN (the pattern or any other), counted on the device."""
        flat = self.t.view(-1)
        return sum(int(torch.isnan(flat[a:a + step]).sum()) for a in range(0, self.n, step))

    def take(self, idx):
        """(values of rows `idx` of the first dimension as f64 on the host, mask of elements that still hold the pattern)."""
        i = torch.as_tensor(idx, device=DEV)
        rows = self.body.view((self.t.shape[0], -1))[i].cpu()
        shape = (len(idx),) + tuple(self.t.shape[1:])
        return rows.view(self.t.dtype).view(shape).double(), (rows == self.pattern).view(shape)


def sources(c, dtype):
    xs = [Big((c.n_img, Hs, Ws, Cs), dtype) for Cs, Hs, Ws, _, _ in c.srcs]
    for k, x in enumerate(xs):
        HC.fill(x.t, HC.SALT_X + k)
    return xs


def panel(c, dtype):
    """(device panel, its host copy) of seeded weights, through ops.pack_weights as in the ABI tests."""
    torch.manual_seed(3000 + sum(map(ord, c.name)))
    fan = c.ktap * c.ktap * sum(s[0] for s in c.srcs)
    w = (torch.randn(IC.weight_shape(c)) * (1.6 / fan ** 0.5)).to(DEV)
    wp = ops.pack_weights(IC.pack_desc(c), w, dtype=dtype)
    assert tuple(wp.shape) == (c.N, c.Ktot)
    return wp, wp.cpu()


def launch_fwd(c, d, dtype):
    shp = int(L.lib.uclstm_igemm_fwd_shape(C.byref(d)))
    assert shp == c.shape, f"{c.name}: dispatches to kernel {shp}, the case is meant for {c.shape}"
    FA.launch(d, dtype, c.name)


def sample_of(h, cuts=()):
    c = h.case
    if c.shape == 3:
        cuts = tuple(cuts) + tuple(HC.ring_block_cuts(c))
    units = HC.sampled_units(c, h.unit, cuts)
    return units, HC.unit_images(units, h.unit)


# ---------------------------------------------------------------------------------------------
# STORE epilogue
# ---------------------------------------------------------------------------------------------
def check_store(name, c, dtype, imgs, wph, bias, outs, stats, ipg):
    """Sampled images of every destination against f64; statistics rows of the sampled groups (`ipg` images each, `imgs` holds
    whole groups in order) against the kernel's own stored values, slot by slot where a slot is one tile, else group sums."""
    ref, mag = IC.gemm_ref(HC.fwd_a(c, imgs, dtype), wph)
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    segs = c.segments()
    ns = len(imgs)
    refs, mags = IC.scatter_segments(ref, ns, c.H, c.W, segs), IC.scatter_segments(mag, ns, c.H, c.W, segs)
    stored = None
    for i, o in enumerate(outs):
        got, untouched = o.take(imgs)
        FA.check_16bit(got, untouched, refs[i], mags[i], dtype, f"{name} segment {i}, {ns} of {c.n_img} images", name)
        keep_worst(name, dtype, FA.WORST, name)
        assert o.pattern_left() == 0, f"{name}: elements of destination {i} were not written"
        assert o.guards_intact(), f"{name}: write outside destination {i}"
        stored = got
    if stats is None:
        return
    assert len(segs) == 1 and segs[0][:4] == (0, c.N, c.N, 0)
    assert stats.pattern_left() == 0 and stats.guards_intact(), f"{name}: statistics rows not written"
    groups = [imgs[k] // ipg for k in range(0, ns, ipg)]
    sgot, _ = stats.take(groups)                                   # [sampled groups][tiles per group][N][2]
    vals = stored.view(len(groups), ipg * c.H * c.W, c.N)
    one = dataclasses.replace(c, n_img=ipg, groups=1)
    tiles = IC.stats_tiles(one)
    assert len(tiles) == sgot.shape[1]
    if c.shape == 3:
        # the ring kernel's persistent blocks merge their consecutive tiles of one group into one slot and zero the others (the
        # consumer adds all slots of a group): the group sums are compared
        tiles = [torch.cat(tiles)]
        sgot = sgot.sum(1, keepdim=True)
    sref = torch.stack([torch.stack((vals[:, p].sum(1), (vals[:, p] ** 2).sum(1)), -1) for p in tiles], 1)
    sabs = torch.stack([torch.stack((vals[:, p].abs().sum(1), (vals[:, p] ** 2).sum(1)), -1) for p in tiles], 1)
    e = float(((sgot - sref).abs() / (sabs + 1e-30)).max())
    print(f"[parity] {name} stats {tag(dtype)}: max |err| / sum|terms| {e:.2e} (<= 2e-6) over {sref.numel()} sums of {len(groups)} groups")
    WORST[(name + " stats", tag(dtype))] = e / 2e-6
    assert e <= 2e-6, f"{name}: statistics slot off by {e:.3e} of sum|terms|"


STORE_PARAMS = [(h.name, BF16) for h in HC.STORE_CASES] + [(n, FP16) for n in HC.FP16_CASES if n.startswith("HF")]


@pytest.mark.parametrize("name,dtype", STORE_PARAMS, ids=[f"{n}-{tag(t)}" for n, t in STORE_PARAMS])
def test_store_epilogue_at_the_top_of_the_descriptor_range(name, dtype):
    h = HC.ALL[name]
    c = h.case
    xs = sources(c, dtype)
    wp, wph = panel(c, dtype)
    torch.manual_seed(7)
    bias = torch.randn(c.N) * 0.5
    bias_d = FA.dev32(bias)
    outs = [Big((c.n_img, s[4], s[5], s[2]), dtype) for s in c.segments()]
    stats = None
    if c.stats:
        tpg = int(L.lib.uclstm_igemm_tiles_per_group(c.n_img, c.H, c.W, c.groups, c.N))
        stats = Big((c.groups, tpg, c.N, 2), torch.float32)
    d = IC.build_desc(c, [x.ptr() for x in xs], wp.data_ptr(), [o.ptr() for o in outs], bias_d.data_ptr(), None, None,
                      stats.ptr() if stats else None)
    launch_fwd(c, d, dtype)
    assert all(x.guards_intact() for x in xs)
    _, imgs = sample_of(h)
    check_store(name, c, dtype, imgs, wph, bias, outs, stats, h.unit)


# ---------------------------------------------------------------------------------------------
# fused cell, split-K slabs and the two group launches
# ---------------------------------------------------------------------------------------------
class Member:
    """One member of a group launch: operands, outputs and descriptor (fresh outputs per instance, the same operands)."""

    def __init__(self, h, dtype, xs=None, wp=None, extra=None):
        self.h, self.c, self.dtype = h, h.case, dtype
        c = self.c
        self.xs = xs if xs is not None else sources(c, dtype)
        self.wp, self.wph = wp if wp is not None else panel(c, dtype)
        src = [x.ptr() for x in self.xs]
        if c.epi == L.EPI_LSTM:
            if extra is None:
                torch.manual_seed(9)
                bias = torch.randn(c.N) * 0.3
                c_prev = Big((c.n_img, c.H, c.W, c.Hd_p), torch.float32)
                HC.fill(c_prev.t, HC.SALT_C)
                extra = (bias, FA.dev32(bias), c_prev)
            self.extra = extra
            M, Hp = c.M, c.Hd_p
            self.outs = [Big((c.n_img, c.H * c.W, Hp), torch.float32), Big((c.n_img, c.H * c.W, Hp), dtype),
                         Big((c.n_img, c.H * c.W, 4, Hp), dtype)]
            self.d = IC.build_desc(c, src, self.wp.data_ptr(), bias=extra[1].data_ptr(), c_prev=extra[2].ptr(), c_out=self.outs[0].ptr(),
                                   h_out=self.outs[1].ptr(), gates_out=self.outs[2].ptr())
        else:
            self.extra = None
            self.used = int(L.lib.uclstm_igemm_ksplit_used(c.Ktot, c.ktap, c.ksplit))
            self.ld = c.N + 8
            self.outs = [Big((self.used, c.n_img, c.H * c.W, self.ld), torch.float32)]
            self.d = IC.build_desc(c, src, self.wp.data_ptr(), acc_out=self.outs[0].ptr(), acc_ld=self.ld, acc_slab=c.M * self.ld)

    def twin(self):
        return Member(self.h, self.dtype, self.xs, (self.wp, self.wph), self.extra)

    def check(self, imgs):
        c, dtype, name = self.c, self.dtype, self.c.name
        A = HC.fwd_a(c, imgs, dtype)
        ns, HW = len(imgs), c.H * c.W
        for o in self.outs:
            assert o.guards_intact(), f"{name}: write outside an output"
        if c.epi == L.EPI_ATOMIC:
            slabs = self.outs[0]
            left = slabs.pattern_left()
            assert left == self.used * c.M * 8, f"{name}: {left} slab elements hold NaN, {self.used * c.M * 8} (the 8 spare columns) should"
            masks = IC.krange_masks(c.ktap, c.ksegs, c.ksplit)
            assert len(masks) == self.used
            rows = slabs.t.view(self.used, c.n_img, HW * self.ld)
            for r, km in enumerate(masks):
                g = rows[r][torch.as_tensor(imgs, device=DEV)].cpu().double().view(ns * HW, self.ld)
                assert bool(torch.isnan(g[:, c.N:]).all()), f"{name}: columns beyond N written"
                ref, mag = IC.gemm_ref(A, self.wph, km)
                FA.check_f32(g[:, :c.N], ref, FA.f32_coeff(c, c.ksplit) * mag, dtype, f"{name} slab {r}, {ns} of {c.n_img} images", name)
                keep_worst(name, dtype, FA.WORST, name)
            return
        # fused cell: the bounds of test_fused_lstm_epilogue_against_f64
        bias, _, c_prev = self.extra
        pre, mag = IC.gemm_ref(A, self.wph)
        pre, mag = pre + bias.double(), mag + bias.double().abs()
        Hp = c.Hd_p
        pre, mag = IC.lstm_rows_to_gates(pre, Hp), IC.lstm_rows_to_gates(mag, Hp)
        cp = c_prev.take(imgs)[0].view(ns * HW, Hp)
        assert torch.equal(cp * 8, HC.values(imgs, HW, Hp, HC.SALT_C).double().view(ns * HW, Hp)) and float(cp.abs().max()) <= 2.0
        gref, cref, href = IC.lstm_cell_ref(pre, cp)
        dpre = FA.f32_coeff(c) * mag
        dg = torch.stack((dpre[:, 0] / 4, dpre[:, 1] / 4, dpre[:, 2], dpre[:, 3] / 4), 1) + FA.E_ACT
        dc = cp.abs() * dg[:, 1] + gref[:, 2].abs() * dg[:, 0] + gref[:, 0].abs() * dg[:, 2] + FA.E_ACT
        for o in self.outs:
            assert o.pattern_left() == 0, f"{name}: elements not written"
        cgot = self.outs[0].take(imgs)[0].view(ns * HW, Hp)
        hgot, hun = self.outs[1].take(imgs)
        ggot, gun = self.outs[2].take(imgs)
        what = f"{ns} of {c.n_img} images"
        FA.check_f32(cgot, cref, dc, dtype, f"{name} c_out, {what}", name + " c_out")
        FA.check_16bit(hgot.view(ns * HW, Hp), hun.view(ns * HW, Hp), href, None, dtype, f"{name} h_out, {what}", name + " h_out",
                       f32_term=dg[:, 3] + dc + FA.E_ACT)
        FA.check_16bit(ggot.view(ns * HW, 4, Hp), gun.view(ns * HW, 4, Hp), gref, None, dtype, f"{name} gates, {what}", name + " gates",
                       f32_term=dg)
        for k in (" c_out", " h_out", " gates"):
            keep_worst(name + k, dtype, FA.WORST, name + k)


@pytest.mark.parametrize("tap", [False, True], ids=["patch-group", "tap-group"])
def test_fused_cell_slabs_and_group_launch_at_the_top_of_the_descriptor_range(tap):
    """uclstm_igemm_fwd_group / uclstm_igemm_fwd_group_tap over a fused cell and a split-K member, both at their image limit; then
    each member as a launch of its own: bit-identical to its part of the group launch over the whole buffers, and the sampled
    images against f64."""
    dtype = BF16
    members = [Member(h, dtype) for h in (HC.GROUP_TAP if tap else HC.GROUP_PATCH)]
    for m in members:
        shp = int(L.lib.uclstm_igemm_fwd_shape(C.byref(m.d)))
        assert shp == m.c.shape == (0 if tap else 2), f"{m.c.name}: kernel {shp}"
    arr = (L.IgemmDesc * len(members))(*[m.d for m in members])
    blocks, entry = (L.lib.uclstm_igemm_fwd_group_tap_blocks, "uclstm_igemm_fwd_group_tap") if tap else \
                    (L.lib.uclstm_igemm_fwd_group_blocks, "uclstm_igemm_fwd_group")
    assert int(blocks(arr, len(members))) > 0
    L.check(getattr(L.kernels(dtype), entry)(arr, len(members), ops._stream()), entry)
    torch.cuda.synchronize()
    for m in members:
        single = m.twin()
        launch_fwd(single.c, single.d, dtype)
        for a, b in zip(single.outs, m.outs):
            assert torch.equal(a.raw, b.raw), f"{m.c.name}: the group launch differs from the single launch"
        assert all(x.guards_intact() for x in single.xs)
        single.check(sample_of(m.h)[1])
        del single
        torch.cuda.empty_cache()
    # atomic mode of the split-K member (acc_slab = 0) onto a pre-loaded accumulator, under the bound of the ABI test
    m = members[1]
    c = m.c
    del m.outs
    torch.cuda.empty_cache()
    acc = Big((c.n_img, c.H, c.W, m.ld), torch.float32)
    HC.fill(acc.t, HC.SALT_C)
    d = IC.build_desc(c, [x.ptr() for x in m.xs], m.wp.data_ptr(), acc_out=acc.ptr(), acc_ld=m.ld, acc_slab=0)
    launch_fwd(c, d, dtype)
    imgs = sample_of(m.h)[1]
    rows = len(imgs) * c.H * c.W
    got = acc.take(imgs)[0].view(rows, m.ld)
    pre = HC.values(imgs, c.H * c.W, m.ld, HC.SALT_C).double().view(rows, m.ld) / 8
    ref, mag = IC.gemm_ref(HC.fwd_a(c, imgs, dtype), m.wph)
    FA.check_f32(got[:, :c.N], ref + pre[:, :c.N], (FA.f32_coeff(c, c.ksplit) + c.ksplit * 2.0 ** -24) * (mag + pre[:, :c.N].abs()), dtype,
                 f"{c.name} atomic, {len(imgs)} of {c.n_img} images", c.name + " atomic")
    keep_worst(c.name + " atomic", dtype, FA.WORST, c.name + " atomic")
    assert torch.equal(got[:, c.N:], pre[:, c.N:]), "columns beyond N of the accumulator changed"
    assert acc.pattern_left() == 0 and acc.guards_intact()


# ---------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------
def window_coeff(c, windows, splits):
    """The bound's coefficient of tests/test_gpu_wgrad_abi.py with the pixels of the windows for M (never larger than its own)."""
    v = max(2e-6, (len(windows) * c.H * c.W / 32 + splits + 2) * 2.0 ** -24)
    assert v <= WA.coeff(c, splits)
    return v


def wgrad_operands(c, windows, dtype, img0=0):
    """Dense sources and dY tensors that are zero outside the window images (indices of the whole tensor; img0: its first image)."""
    xs = [Big((c.n_img, Hs, Ws, Cs), dtype) for Cs, Hs, Ws, _, _ in c.srcs]
    for k, x in enumerate(xs):
        HC.fill(x.t, HC.SALT_X + k, img0)
    dys = [Big((c.n_img, Hd, Wd, Cd), dtype) for Cd, Hd, Wd in c.dy_tensors()]
    w = torch.as_tensor(windows, device=DEV)
    for k, t in enumerate(dys):
        t.t.zero_()
        v = HC.values(w + img0, t.t.shape[1] * t.t.shape[2], t.t.shape[3], HC.SALT_DY + k, DEV)
        t.t[w] = (v.to(torch.float32) / 8).to(dtype).view((len(windows),) + tuple(t.t.shape[1:]))
    return xs, dys


def panel_to_weight(p, cs, ktap):
    """[N][Ktot] in the header's K order -> OIHW [N][sum(cs)][ktap][ktap] (the inverse of igemm_cases.host_panel)."""
    ksegs = [IC.roundup(c, 64) for c in cs]
    kt = sum(ksegs)
    w = torch.zeros(p.shape[0], sum(cs), ktap, ktap, dtype=p.dtype)
    for t in range(ktap * ktap):
        base, ch = t * kt, 0
        for c, ks in zip(cs, ksegs):
            w[:, ch:ch + c, t // ktap, t % ktap] = p[:, base:base + c]
            base, ch = base + ks, ch + c
    return w


WGRAD_PARAMS = [(h.name, BF16) for h in HC.WGRAD_CASES] + [(n, FP16) for n in HC.FP16_CASES if n.startswith("HW")]


@pytest.mark.parametrize("name,dtype", WGRAD_PARAMS, ids=[f"{n}-{tag(t)}" for n, t in WGRAD_PARAMS])
def test_weight_gradient_at_the_top_of_the_descriptor_range(name, dtype):
    """Slab mode with the library's own plan (every slab written, the spare slab and the guards untouched, the f64 sum of the
    slabs against the window reference), the unpack of those slabs into the OIHW gradient, and atomic mode onto a pre-loaded
    panel."""
    h = HC.ALL[name]
    c = h.case
    shape, splits = HC.wgrad_plan(c)
    windows = HC.wgrad_windows(h, splits)
    xs, dys = wgrad_operands(c, windows, dtype)
    ref, mag = HC.wgrad_window_ref(c, windows, dtype)
    panel_elems = c.N * c.Ktot
    d = WC.build_wgrad_desc(c, [x.ptr() for x in xs], [t.ptr() for t in dys])
    assert WC.wgrad_shape(d) == c.shape == shape, f"{name}: dispatches to kernel {WC.wgrad_shape(d)}, meant for {c.shape}"
    used = WC.wgrad_splits(d)
    assert used == splits, f"{name}: {used} ranges with real pointers, {splits} with dummies: the windows miss the boundaries"
    d.splits = used
    buf = WA.Guarded(used + 1, panel_elems)
    d.dwp = buf.ptr()
    assert WA.launch(d, dtype) == 0, name
    got, untouched = buf.read()
    expect = torch.ones_like(untouched)
    expect[:used] = False
    assert torch.equal(untouched, expect), f"{name}: {int((untouched & ~expect).sum())} slab elements not written, " \
                                           f"{int((~untouched & expect).sum())} written beyond the {used} slabs"
    slabs = got[:used].reshape(used, c.N, c.Ktot)
    assert bool((slabs[:, mag == 0] == 0).all()), f"{name}: a structural zero of some slab is not exactly 0"
    coef = window_coeff(c, windows, used)
    key = f"{c.shape} {name}"
    WA.check_panel(slabs.sum(0), ref, mag, None, coef, dtype, f"{name} ({used} slabs, {len(windows)} window images of {c.n_img})", key)
    keep_worst(name + " slabs", dtype, WA.WORST, f"wgrad kernel {key}")
    # sharper than the bound, from the number formats alone: every product is a multiple of 2^-6 and every partial sum is below
    # mag < 2^18, so f32 accumulation in any order, and the f64 sum of the slabs, are exact -- one dropped or doubled pixel shows
    assert float(mag.max()) < 2.0 ** 18
    assert torch.equal(slabs.sum(0), ref), f"{name}: {int((slabs.sum(0) != ref).sum())} panel elements differ from the exact sum"
    assert all(t.guards_intact() for t in xs + dys)
    # the unpack of the slabs: OIHW gradient of the convolution this launch differentiates
    cs = [s[0] for s in c.srcs]
    like = torch.empty(c.N, sum(cs), c.ktap, c.ktap, device=DEV)
    grad = ops.unpack_wgrad(ops.conv_pack_desc(c.N, sum(cs), cs, cs, c.ktap), buf.t[:used].view(used, c.N, c.Ktot), like)
    torch.cuda.synchronize()
    WA.check_panel(grad.cpu().double().view(c.N, -1), panel_to_weight(ref, cs, c.ktap).view(c.N, -1),
                   panel_to_weight(mag, cs, c.ktap).view(c.N, -1), None, coef, dtype, f"{name} unpacked", key + " unpack")
    keep_worst(name + " unpacked", dtype, WA.WORST, f"wgrad kernel {key} unpack")
    # atomic mode onto a pre-loaded panel (the ring kernel is slab-only: the descriptor then takes another kernel)
    pre = torch.randn(c.N, c.Ktot, generator=torch.Generator().manual_seed(11))
    d = WC.build_wgrad_desc(c, [x.ptr() for x in xs], [t.ptr() for t in dys], slab=0)
    kernel = c.atomic_shape if c.shape == 4 else c.shape
    assert WC.wgrad_shape(d) == kernel
    ranges = WC.wgrad_splits(d)
    acc = WA.Guarded(1, panel_elems)
    acc.load(pre)
    d.dwp, d.splits = acc.ptr(), ranges
    if ranges != used or kernel != c.shape:
        # another plan: its boundaries need their own windows, and dY must be zero outside them
        windows = HC.wgrad_windows(dataclasses.replace(h, case=dataclasses.replace(c, shape=kernel)), ranges)
        del xs, dys
        torch.cuda.empty_cache()
        xs, dys = wgrad_operands(c, windows, dtype)
        ref, mag = HC.wgrad_window_ref(c, windows, dtype)
        for i, x in enumerate(xs):
            d.src[i].ptr = x.ptr()
        for i, (_, _, ti, _, _, _, _) in enumerate(c.segments()):
            d.seg[i].ptr = dys[ti].ptr()
    assert WA.launch(d, dtype) == 0, name
    got, untouched = acc.read()
    assert not bool(untouched.any())
    got = got.view(c.N, c.Ktot)
    assert torch.equal(got[mag == 0], pre.double()[mag == 0]), f"{name}: a structural zero changed the pre-loaded panel"
    WA.check_panel(got, ref, mag, pre, window_coeff(c, windows, ranges), dtype, f"{name} atomic ({ranges} ranges)", key + " atomic")
    keep_worst(name + " atomic", dtype, WA.WORST, f"wgrad kernel {key} atomic")


# ---------------------------------------------------------------------------------------------
# through ops, with the real LAUNCH_BYTES_LIMIT
# ---------------------------------------------------------------------------------------------
OPS_N = 4096                             # 4096 images of 64 x 64 x 64 16-bit channels: exactly 2^31 bytes
OPS_CASE = IC.Case("ops-2GiB", 3, OPS_N, 64, 64, [(64, 64, 64, 0, 0)], 64)


@pytest.fixture
def launch_log():
    ops.LAUNCH_LOG = []
    yield ops.LAUNCH_LOG
    ops.LAUNCH_LOG = None


@pytest.mark.parametrize("with_stats", [False, True], ids=["image-cuts", "group-cuts"])
def test_igemm_store_cuts_a_tensor_of_2_gib(with_stats, launch_log):
    """ops.igemm_store on exactly 2^31 bytes: without statistics the launch is cut at an image, with statistics at a BatchNorm
    group of 2 images; both sides of the cut are among the sampled images."""
    dtype = BF16
    groups = 2048 if with_stats else 1
    ipg = OPS_N // groups if with_stats else 1                # what a cut is a multiple of
    c = dataclasses.replace(OPS_CASE, groups=groups, stats=with_stats)
    assert c.n_img * c.H * c.W * 64 * 2 == 1 << 31
    assert HC.fwd_shape(c) == HC.E_BADARG                      # the library refuses the tensor as one launch
    chunks = ops._img_chunks(OPS_N, groups, 64 * 64 * 64 * 2, "test", whole_groups=with_stats)
    assert len(chunks) == 2 and chunks[0][1] % ipg == 0
    xs = sources(c, dtype)
    wp, wph = panel(c, dtype)
    torch.manual_seed(7)
    bias = torch.randn(c.N) * 0.5
    bias_d = FA.dev32(bias)
    out = Big((OPS_N, 64, 64, 64), dtype)
    stats = None
    if with_stats:
        stats = Big((groups, int(L.lib.uclstm_igemm_tiles_per_group(OPS_N, 64, 64, groups, 64)), 64, 2), torch.float32)
    ops.igemm_store([ops.SrcView(xs[0].t)], wp, (64, 64), OPS_N, [(out.t, 0, 64, 0, 1, 0, 0)], ktap=3, pad=1, groups=groups, bias=bias_d,
                    stats=stats.t if with_stats else None)
    torch.cuda.synchronize()
    assert ("split", "igemm_fwd(store)", 2) in launch_log
    assert [e[2] for e in launch_log if e[0] == "fwd"] == [3, 3], launch_log
    assert xs[0].guards_intact()
    units =HC.sampled_units(c, ipg, [chunks[0][1]])
    assert chunks[0][1] // ipg in units and chunks[0][1] // ipg - 1 in units
    name = "ops igemm_store " + ("group cuts" if with_stats else "image cuts")
    check_store(name, c, dtype, HC.unit_images(units, ipg), wph, bias, [out], stats, ipg)


def test_igemm_wgrad_cuts_operands_of_2_gib(launch_log):
    """ops.igemm_wgrad on operands of exactly 2^31 bytes: two launches, their slabs side by side; the windows hold both sides of
    the cut."""
    dtype = BF16
    c = WC.WCase("ops-2GiB-wgrad", 4, OPS_N, 64, 64, [(64, 64, 64, 0, 0)], 64)
    assert HC.wgrad_plan(c)[0] == 0                                # as one launch the operands would leave the fast paths
    chunks = ops._img_chunks(OPS_N, 1, 64 * 64 * 64 * 2, "test")
    assert len(chunks) == 2
    windows = HC.sampled_units(c, 1, [chunks[0][1]])
    assert chunks[0][1] in windows and chunks[0][1] - 1 in windows
    xs, dys = wgrad_operands(c, windows, dtype)
    dwp = ops.igemm_wgrad([ops.SrcView(xs[0].t)], [(dys[0].t, 0, 64, 0, 1, 0, 0)], 64, 576, (64, 64), OPS_N, ktap=3, pad=1)
    torch.cuda.synchronize()
    assert ("split", "igemm_wgrad", 2) in launch_log
    plans = [e for e in launch_log if e[0] == "wgrad"]
    assert [e[1] for e in plans] == [4, 4] and dwp.shape[0] == sum(e[4] for e in plans), plans
    ref, mag = HC.wgrad_window_ref(c, windows, dtype, batch=2)
    got = dwp.cpu().double()
    assert bool(torch.isfinite(got).all())
    WA.check_panel(got.sum(0), ref, mag, None, window_coeff(c, windows, dwp.shape[0]), dtype,
                   f"ops igemm_wgrad ({dwp.shape[0]} slabs of two launches)", "4 ops")
    keep_worst("ops igemm_wgrad", dtype, WA.WORST, "wgrad kernel 4 ops")
    assert float(mag.max()) < 2.0 ** 18 and torch.equal(got.sum(0), ref), "the slabs do not add up to the exact sum"
    assert all(t.guards_intact() for t in xs + dys)


def test_convlstm_x_half_cuts_pre_activations_of_2_gib(launch_log):
    """The hoisted W_x * x_t of a ConvLSTM layer (ops._LstmLayerFwd, hoist=True): T*B = 32768 images of 16 x 16 with Hd = 16 make
    f32 pre-activations of exactly 2^31 bytes, which the layer's own _img_chunks call cuts into two slab launches."""
    dtype = BF16
    T, B, H, W, Cx, Hd = 2, 16384, 16, 16, 8, 16
    torch.manual_seed(13)
    weight = (torch.randn(4 * Hd, Cx + Hd, 3, 3) * (1.6 / (9 * (Cx + Hd)) ** 0.5)).to(DEV)
    wx = ops.pack_weights(ops.lstm_half_pack_desc(Hd, Cx, "x", 3), weight, 0, dtype)
    N = wx.shape[0]
    assert T * B * H * W * N * 4 == 1 << 31
    chunks = ops._img_chunks(T * B, 1, H * W * N * 4, "test")
    assert len(chunks) == 2
    x = Big((T * B, H, W, Cx), dtype)
    HC.fill(x.t, HC.SALT_X)
    poison = torch.full((T * B * H * W * N,), float("nan"), device=DEV)      # best effort: the layer's torch.empty may reuse it
    del poison
    layer = ops._LstmLayerFwd(x.t.view(T, B, H, W, Cx), None, None, weight, None, Hd, Cx, False, hoist=True)
    torch.cuda.synchronize()
    launches = [e for e in launch_log if e[0] == "fwd" and e[1] == L.EPI_ATOMIC]
    assert len(launches) == 2 and all(e[2] == 1 for e in launches), launch_log
    assert x.guards_intact()
    c = IC.Case("ops convlstm x half", 1, T * B, H, W, [(Cx, H, W, 0, 0)], N, epi=L.EPI_ATOMIC, bias=False)
    imgs = HC.sampled_units(c, 1, [chunks[0][1]])
    assert chunks[0][1] in imgs and chunks[0][1] - 1 in imgs
    ref, mag = IC.gemm_ref(HC.fwd_a(c, imgs, dtype), wx.cpu())
    pre = layer.pre_x.view(T * B, H * W * N)
    assert not bool(torch.isnan(pre).any()), "pre-activations not written"
    got = pre[torch.as_tensor(imgs, device=DEV)].cpu().double().view(len(imgs) * H * W, N)
    FA.check_f32(got, ref, FA.f32_coeff(c, 1) * mag, dtype, f"convlstm x half, {len(imgs)} of {T * B} images", c.name)
    keep_worst(c.name, dtype, FA.WORST, c.name)
