"""tests/high_offset_cases.py without a GPU: the validation-only entry points take dummy pointers, so the dispatch of every case
at its real size, the boundary it sits at, the selection rules, the data generator and the sampled f64 references are all
checked here; tests/test_gpu_high_offset.py then only has to launch."""
import dataclasses

import pytest
import torch

import high_offset_cases as HC
import igemm_cases as IC
import wgrad_cases as WC
from unet_convlstm_amd import ops

L = IC.L
FWD = [h.name for h in HC.FWD_CASES]
WGRAD = [h.name for h in HC.WGRAD_CASES]


def group_blocks(members, tap):
    arr = (L.IgemmDesc * len(members))(*[IC.dummy_desc(c) for c in members])
    fn = L.lib.uclstm_igemm_fwd_group_tap_blocks if tap else L.lib.uclstm_igemm_fwd_group_blocks
    return int(fn(arr, len(members)))


# ---------------------------------------------------------------------------------------------
# every case runs the kernel it is meant for, at the boundary of that kernel's launch conditions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FWD)
def test_forward_case_sits_at_its_boundary(name):
    h = HC.ALL[name]
    c = h.case
    assert HC.fwd_shape(c) == c.shape, f"{name}: kernel {HC.fwd_shape(c)}, meant for {c.shape}"
    assert HC.fwd_shape(h.with_images(c.n_img + h.unit)) == h.over, f"{name}: one more unit is not refused"
    top = max(c.n_img * p + HC.fwd_bias(s, c.pad) for p, s in zip(HC.operand_bytes_per_image(c), c.srcs))
    assert (1 << 31) - (1 << 23) < top < HC.DESC_LIMIT, f"{name}: the largest operand ends at byte {top}"


def test_the_example_of_the_64_channel_64x64_image():
    """64 x 64 x 64 images are 512 KiB: plan_fwd and the ring kernel's condition accept 4087 of them and refuse 4088."""
    src = [(64, 64, 64, 0, 0)]
    assert HC.fwd_max_images(src, 1) == 4087
    c = IC.Case("ring-64x64", 3, 4087, 64, 64, src, 64)
    assert HC.fwd_shape(c) == 3
    assert HC.fwd_shape(dataclasses.replace(c, n_img=4088)) == HC.E_BADARG


def test_destinations_may_exceed_the_descriptor_range():
    for name, crossed in (("HF0-n160", 1 << 32), ("HF4-k1-n128", 1 << 31)):
        c = HC.ALL[name].case
        assert c.M * c.N * 2 > crossed and HC.fwd_shape(c) == c.shape


def test_flat_kernel_hands_over_a_destination_of_2_to_the_31_pixels():
    """The flat kernel indexes destination pixels with 32 bits: the same launch with a destination grid of 2^31 pixels and more
    takes the per-tap loop, which builds 64-bit store offsets."""
    src = [(8, 16, 16, 0, 0)]
    n = 1 << 17
    fits = [(0, 128, 128, 0, 127, 128, 1, 0, 0)]             # n * 127 * 128 < 2^31 destination pixels
    over = [(0, 128, 128, 0, 128, 128, 1, 0, 0)]             # n * 128 * 128 = 2^31
    assert HC.fwd_shape(IC.Case("flat", 4, n, 16, 16, src, 128, ktap=1, pad=0, segs=fits)) == 4
    assert HC.fwd_shape(IC.Case("flat", 0, n, 16, 16, src, 128, ktap=1, pad=0, segs=over)) == 0


def test_padded_index_limits_of_ring_and_patch_lie_beyond_the_byte_limit():
    """c64_ok asks n_img*(W/64)*(H+1) < 2^30 and patch_ok n_img*(H+1)*(W+1) < 2^30.  Their sources have at least 64 channels, so
    the byte limit caps n_img*H*W below 2^24, and (H+1)/(64*H) <= 1/32 resp. (H+1)*(W+1)/(H*W) <= 4 keep both products below
    2^26: the cases at the byte limit are at the only limit these kernels can meet."""
    pixels = HC.DESC_LIMIT // 128
    assert pixels < 1 << 24 and 4 * pixels < 1 << 30
    for name in ("HF3-ring", "HF2-tile", "HF2-strip"):
        c = HC.ALL[name].case
        assert c.n_img * (c.H + 1) * (c.W + 1) < 1 << 26 and c.n_img * max(1, c.W // 64) * (c.H + 1) < 1 << 26


def test_group_launches_accept_the_cases_at_their_limit():
    """Both group entry points take the fused-cell and the slab member at full size and refuse them with one more image."""
    for members, tap in ((HC.GROUP_PATCH, False), (HC.GROUP_TAP, True)):
        cases = [h.case for h in members]
        assert len({len(c.srcs) for c in cases}) == 1
        assert group_blocks(cases, tap) > 0
        assert group_blocks(cases, not tap) == HC.E_BADARG
        for k in range(len(cases)):
            more = [h.with_images(h.case.n_img + 1) if i == k else h.case for i, h in enumerate(members)]
            assert group_blocks(more, tap) == HC.E_BADARG


@pytest.mark.parametrize("name", WGRAD)
def test_weight_gradient_case_sits_at_its_boundary(name):
    h = HC.ALL[name]
    c = h.case
    shape, splits = HC.wgrad_plan(c)
    assert shape == c.shape and splits >= 1, f"{name}: kernel {shape}, meant for {c.shape}"
    assert HC.wgrad_plan(h.with_images(c.n_img + 1))[0] == h.over, f"{name}: one more image neither refused nor re-routed"
    per = HC.operand_bytes_per_image(c)
    if c.shape == 0:
        # generic addressing: operands between 2^31 bytes and 2^31 elements
        assert all(c.n_img * p > (1 << 31) for p in per) and max(c.n_img * p // 2 for p in per) < HC.WGRAD_ELEMS
        if name == "HW0-beyond":
            fast = WC.WCase("fast", 1, HC.ALL["HW1"].case.n_img, c.H, c.W, c.srcs, c.N)
            assert HC.wgrad_plan(fast)[0] == 1 and HC.wgrad_plan(dataclasses.replace(fast, n_img=fast.n_img + 1))[0] == 0
    else:
        assert (1 << 31) - (1 << 23) < max(c.n_img * p for p in per) < HC.DESC_LIMIT
    if h.walk is not None:
        assert HC.walks(c) == h.walk
    if c.shape == 4:
        # atomic mode is not the ring kernel's: the same descriptor takes the buffer-addressed kernel
        assert HC.wgrad_plan(c, slab=0)[0] == c.atomic_shape


def test_the_walk_pixel_limit_lies_beyond_the_byte_limit():
    """wgrad_run walks valid pixels only below 2^24 - 4096 pixels.  A 256 x 256 launch reads dY rows of at least 512 bytes, so the
    byte limit of the fast path caps it near 2^22 pixels: no admissible launch reaches the pixel limit, and `without the walk`
    is the launch whose K tiles straddle taps."""
    assert HC.DESC_LIMIT // (256 * 2) < (1 << 24) - 4096
    c = HC.ALL["HW3-walk"].case
    assert c.M == HC.wgrad_fast_max_images(c) * 256 < HC.DESC_LIMIT // 512


# ---------------------------------------------------------------------------------------------
# selection rules
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FWD)
def test_sampled_images_hold_the_required_offsets(name):
    h = HC.ALL[name]
    c = h.case
    cuts = HC.ring_block_cuts(c) if c.shape == 3 else ()
    units = HC.sampled_units(c, h.unit, cuts)
    imgs = set(HC.unit_images(units, h.unit))
    assert len(imgs) >= 16 and units == HC.sampled_units(c, h.unit, cuts) and max(imgs) == c.n_img - 1 and min(imgs) == 0
    req = HC.required_images(c)
    assert sum(k.startswith("operand") for k in req) >= 2, "no operand reaches 2^31 - 2^23 bytes"
    for what, img in req.items():
        assert img in imgs, f"{name}: {what} (image {img}) is not sampled"
    for k, per in enumerate(HC.operand_bytes_per_image(c)):
        for off in HC.OFFSETS:
            if off < c.n_img * per:
                assert req[f"operand {k} byte {off}"] * per <= off < (req[f"operand {k} byte {off}"] + 1) * per
    for cut in cuts:
        assert cut in imgs and cut - 1 in imgs


@pytest.mark.parametrize("name", WGRAD)
def test_windows_cover_every_pixel_range_boundary(name):
    h = HC.ALL[name]
    c = h.case
    _, splits = HC.wgrad_plan(c)
    windows = HC.wgrad_windows(h, splits)
    w = set(windows)
    for what, img in HC.required_images(c).items():
        assert img in w, f"{name}: {what} (image {img}) is outside the windows"
    bounds = HC.wgrad_boundary_images(h, splits)
    assert len(bounds) >= min(splits - 1, 1)
    for b in bounds:
        assert b in w and (b == 0 or b - 1 in w), f"{name}: boundary image {b}"
    if c.shape != 4:
        # the ranges as wgrad_run cuts them: `splits` ranges of `chunk` pixels cover M, and splits - 1 do not
        chunk = IC.roundup(-(-c.M // splits), 64)
        assert (splits - 1) * chunk < c.M <= splits * chunk
    pixels = len(windows) * c.H * c.W
    print(f"[high-offset] {name}: {c.n_img} images, {splits} ranges, {len(windows)} window images, {pixels} pixels")
    assert pixels * c.N * c.Ktot * 2 < 60e9, "the window reference would take more than a couple of seconds"


# ---------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------
def test_generator_host_form_equals_whole_tensor_form():
    n, Hs, Ws, ch = 37, 5, 6, 24
    for dtype in (torch.bfloat16, torch.float16):
        whole = torch.empty(n, Hs, Ws, ch, dtype=dtype)
        HC.fill(whole, 3, chunk_elems=4000)                     # several chunks
        assert torch.equal(whole, HC.host_images(list(range(n)), Hs, Ws, ch, 3, dtype))
        pick = [36, 0, 17]
        assert torch.equal(whole[pick], HC.host_images(pick, Hs, Ws, ch, 3, dtype))
        shifted = torch.empty(4, Hs, Ws, ch, dtype=dtype)
        HC.fill(shifted, 3, img0=20)
        assert torch.equal(shifted, whole[20:24])
        assert torch.equal(whole.double() * 8, HC.values(range(n), Hs * Ws, ch, 3).view(n, Hs, Ws, ch).double())       # exact in 16 bits
    v = HC.values(range(64), 256, 64, 1)
    assert int(v.min()) == -7 and int(v.max()) == 7 and abs(float(v.double().mean())) < 0.05
    assert not torch.equal(HC.values(range(4), 30, 24, 3), HC.values(range(4), 30, 24, 4))


@pytest.mark.parametrize("name", FWD + WGRAD)
def test_generator_has_no_period_of_a_power_of_two_bytes(name):
    """An address off by 2^30, 2^31 or 2^32 bytes lands a whole number of images away: those images differ almost everywhere."""
    c = HC.ALL[name].case
    for k, ((Cs, Hs, Ws, _, _), per) in enumerate(zip(c.srcs, HC.operand_bytes_per_image(c))):
        for off in (1 << 30, 1 << 31, 1 << 32):
            d = off // per
            a, b = HC.values([0, 5, d + 7], Hs * Ws, Cs, HC.SALT_X + k), HC.values([d, d + 5, 2 * d + 7], Hs * Ws, Cs, HC.SALT_X + k)
            assert float((a != b).double().mean()) > 0.85, f"{name}: source {k} repeats after {off} bytes"


# ---------------------------------------------------------------------------------------------
# Python and C agree at the real LAUNCH_BYTES_LIMIT
# ---------------------------------------------------------------------------------------------
def test_every_range_of_img_chunks_is_accepted_by_the_library():
    """Tensors of 2^31 bytes and more over a sweep of image sizes and channel counts, wide images (the largest descriptor bias)
    among them: every image range ops._img_chunks returns, with and without whole BatchNorm groups, passes plan_fwd, and the
    weight-gradient plan keeps it on the fast path."""
    assert ops.LAUNCH_BYTES_LIMIT == (1 << 31) - (1 << 23)
    checked = 0
    for H, W in ((16, 16), (64, 64), (4, 1024), (256, 256), (8, 4096), (512, 512)):
        for ch in (8, 64, 72, 256):
            per = H * W * ch * 2
            if 8 * per >= ops.LAUNCH_BYTES_LIMIT:
                continue
            for total in ((1 << 31), (1 << 31) + (1 << 30)):
                n = -(-total // per // 8) * 8
                for whole_groups in (False, True):
                    chunks = ops._img_chunks(n, n // 8, per, "sweep", whole_groups=whole_groups)
                    assert len(chunks) >= 2 and chunks[0][0] == 0 and chunks[-1][1] == n
                    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
                    for i0, i1 in {chunks[0], chunks[-1]}:
                        m = i1 - i0
                        assert m * per < ops.LAUNCH_BYTES_LIMIT and (not whole_groups or m % 8 == 0)
                        src = [(ch, H, W, 0, 0)]
                        assert HC.fwd_shape(IC.Case("sweep", 0, m, H, W, src, 64, groups=m // 8 if whole_groups else 1)) >= 0, (H, W, ch, m)
                        # a shifted source of the same size: pad + offset of 2 rows and 2 columns, the bias of a 5x5 on this width
                        assert HC.fwd_shape(IC.Case("sweep", 0, m, H, W, [(ch, H, W, 1, 1)], 64)) >= 0, (H, W, ch, m)
                        kernel, splits = HC.wgrad_plan(WC.WCase("sweep", 0, m, H, W, src, ch))
                        assert kernel > 0 and splits >= 1, (H, W, ch, m, kernel)
                        checked += 1
    assert checked >= 60


# ---------------------------------------------------------------------------------------------
# the sampled references against dense f64 references, at the cases' image sizes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FWD)
def test_sampled_forward_reference_equals_the_dense_one(name):
    """The A operand of a subset of images is the subset of rows of the dense A operand (all images of a small launch)."""
    h = HC.ALL[name]
    c = h.with_images(5 * h.unit)
    dense = HC.fwd_a(c, list(range(c.n_img)), torch.bfloat16).view(c.n_img, c.H * c.W, -1)
    pick = [4, 0, 2]
    assert torch.equal(HC.fwd_a(c, pick, torch.bfloat16).view(3, c.H * c.W, -1), dense[pick])
    assert float((dense != 0).double().mean()) > 0.3


@pytest.mark.parametrize("name", WGRAD)
def test_window_reference_equals_the_dense_one(name):
    """dY = 0 outside the windows: the sum over the windows is the dense weight gradient of the masked dY, to f64 rounding."""
    c = dataclasses.replace(HC.ALL[name].case, n_img=7)
    windows = [0, 3, 4, 6]
    ref, mag = HC.wgrad_window_ref(c, windows, torch.bfloat16, batch=3)
    imgs = list(range(c.n_img))
    xs = [(HC.host_images(imgs, Hs, Ws, Cs, HC.SALT_X + k, torch.bfloat16), oy, ox) for k, (Cs, Hs, Ws, oy, ox) in enumerate(c.srcs)]
    dys = [HC.host_images(imgs, Hd, Wd, Cd, HC.SALT_DY + k, torch.bfloat16) for k, (Cd, Hd, Wd) in enumerate(c.dy_tensors())]
    for t in dys:
        t[[i for i in imgs if i not in windows]] = 0
    dense, dmag = WC.wgrad_ref(c.n_img, c.H, c.W, c.N, c.ktap, c.scale, c.pad, xs,
                               [(dys[ti], n0, n1, co, sc, oy, ox) for n0, n1, ti, co, sc, oy, ox in c.segments()])
    assert float((ref - dense).abs().max()) <= 1e-12 * float(dmag.max()) and float((mag - dmag).abs().max()) <= 1e-12 * float(dmag.max())
    assert float(mag.min()) > 0
