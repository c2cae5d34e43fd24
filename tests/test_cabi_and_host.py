"""CPU-only tests: the C-ABI library loads and exports every symbol of include/uclstm.h, argument contracts are
enforced before any launch, the host-side mirror keeps the reference's module surface, and the flat-buffer
data-parallel path is correct with world_size 2 on gloo.  No kernel is launched here."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_golden, sub

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops
from unet_convlstm_amd.optim import FlatParams
from unet_convlstm_amd.ddp import FlatDDP


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def test_library_exports_every_header_symbol():
    syms = L.header_symbols()
    assert len(syms) >= 29
    bound = set(L._PROTOS) | {n + "_f16" for n in L.F16_TWINS}          # the fp16 twins share their prototype's binding
    assert set(syms) == bound, (set(syms) ^ bound)
    assert len(L.F16_TWINS) == 29 and all(n in L._PROTOS for n in L.F16_TWINS)
    assert L.kernels(torch.bfloat16) is L.lib and L.kernels(torch.float16).uclstm_igemm_fwd is not L.lib.uclstm_igemm_fwd
    assert L.kernels(torch.float16).uclstm_bn_finalize is L.lib.uclstm_bn_finalize            # shared (f32-only) entry point
    raw = C.CDLL(L.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
    hdr = open(L.HEADER_PATH).read()
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == int(re.search(r"#define UCLSTM_ABI_VERSION (\d+)", hdr).group(1))
    assert L.lib.uclstm_build_arch() == b"gfx950"


def test_library_reports_the_sources_of_this_tree():
    """Ship exactly what is tracked: the loaded library was built from csrc/*, include/uclstm.h and build.py's flags as they are
    in this tree (the loader would have refused it otherwise), and the sidecar binds that hash to this very file."""
    from unet_convlstm_amd import build as B
    assert L.lib.uclstm_source_hash().decode() == B.source_hash()
    assert B.library_hash(L.LIB_PATH) == B.source_hash() and not B.needs_rebuild()
    stray = [f for f in os.listdir(os.path.join(ROOT, "unet-convlstm_amd", "build")) if f.endswith(".so") or "whatif" in f] \
        if os.path.isdir(os.path.join(ROOT, "unet-convlstm_amd", "build")) else []
    assert not stray, f"stale A/B builds would ship to the GPU box: {stray} (keep them under unet-convlstm_amd/ab/)"


def test_build_recompiles_when_a_source_byte_changes(tmp_path):
    """build() decides by content hash, not by mtime: an edited source byte (with the old mtime restored) recompiles, an
    untouched tree does not, and a library next to a foreign sidecar counts as stale."""
    from unet_convlstm_amd import build as B
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    hdr = tmp_path / "api.h"
    hdr.write_text("int probe_value(void);\n")
    src = csrc / "probe.hip"
    src.write_text('#include <hip/hip_runtime.h>\n__global__ void k(int* p) { *p = 1; }\nextern "C" int probe_value(void) { return 41; }\n')
    lib = str(tmp_path / "libprobe.so")
    kw = dict(csrc=str(csrc), header=str(hdr), lib=lib, sources=["probe.hip"], f16_sources=[], verbose=False)
    B.build(**kw)
    h0 = B.source_hash(str(csrc), str(hdr), ["probe.hip"], [])
    so = C.CDLL(lib)
    so.uclstm_source_hash.restype = C.c_char_p
    assert so.uclstm_source_hash().decode() == h0 == B.library_hash(lib) and so.probe_value() == 41
    t_lib, t_obj = os.path.getmtime(lib), os.path.getmtime(tmp_path / "build" / "probe.o")
    B.build(**kw)                                                    # nothing changed: nothing rebuilt
    assert os.path.getmtime(lib) == t_lib and os.path.getmtime(tmp_path / "build" / "probe.o") == t_obj
    st = os.stat(src)
    src.write_text(src.read_text().replace("return 41", "return 42"))
    os.utime(src, (st.st_atime, st.st_mtime))                        # an mtime-based check would not see this edit
    assert B.needs_rebuild(lib, str(csrc), str(hdr), ["probe.hip"], [])
    B.build(**kw)
    h1 = B.source_hash(str(csrc), str(hdr), ["probe.hip"], [])
    assert h1 != h0 and B.library_hash(lib) == h1
    lib2 = str(tmp_path / "libprobe2.so")                            # dlopen caches by path: load the rebuilt file under a new name
    os.link(lib, lib2)
    so2 = C.CDLL(lib2)
    so2.uclstm_source_hash.restype = C.c_char_p
    assert so2.uclstm_source_hash().decode() == h1 and so2.probe_value() == 42
    with open(lib, "ab") as f:                                       # a library that is not the one the sidecar describes
        f.write(b"\0")
    assert B.library_hash(lib) is None and B.needs_rebuild(lib, str(csrc), str(hdr), ["probe.hip"], [])


def test_struct_layouts_match_the_header():
    # sizes follow from the header's field lists (natural alignment, 8-byte pointers)
    assert C.sizeof(L.Src) == 32
    assert C.sizeof(L.Seg) == 48
    assert C.sizeof(L.PackDesc) == 4 * 17 + 4 + 8 * 4      # 17 ints (+4 pad) + 4 int64
    d = L.IgemmDesc()
    assert C.sizeof(d) % 8 == 0 and type(d).src.offset == 32 and type(d).wp.offset == 96
    # v7: pre_add sits between the LSTM outputs and the split-K block
    assert type(d).pre_add.offset == type(d).gates_out.offset + 8 and type(d).acc_out.offset == type(d).pre_add.offset + 8
    h = ops.lstm_half_pack_desc(40, 24, "h")
    x = ops.lstm_half_pack_desc(40, 24, "x")
    full = ops.lstm_pack_desc(40, 24)
    assert h.N == x.N == full.N and h.Ktot + x.Ktot == full.Ktot and (h.choff[0], x.choff[0]) == (24, 0)


def test_argument_contracts_are_checked_before_launch():
    # null / malformed descriptors must come back as UCLSTM_E_BADARG (-1) without touching a device
    assert L.lib.uclstm_igemm_fwd(None, None) == -1
    assert L.lib.uclstm_igemm_wgrad(None, None) == -1
    d = L.IgemmDesc()
    d.n_img, d.H, d.W, d.groups, d.ktap, d.scale, d.pad, d.nsrc = 4, 8, 8, 3, 3, 1, 1, 1      # 4 % 3 != 0
    assert L.lib.uclstm_igemm_fwd(C.byref(d), None) == -1
    assert L.lib.uclstm_igemm_tiles_per_group(4, 8, 8, 3, 128) == -1
    assert L.lib.uclstm_igemm_tiles_per_group(640, 64, 64, 20, 128) == 1024     # 128 x 128-pixel blocks
    assert L.lib.uclstm_igemm_tiles_per_group(640, 64, 64, 20, 64) == 512       # narrow panel: 64 x 256-pixel blocks
    assert L.lib.uclstm_igemm_tiles_per_group(4, 8, 8, 1, 128) == 2             # small layer: 128 x 128-pixel blocks
    assert L.lib.uclstm_bn_apply_relu(None, None, None, None, 10, 10, 8, None) == -1
    assert L.lib.uclstm_maxpool2_fwd(None, None, 1, 4, 4, 8, None) == -1
    assert L.lib.uclstm_adamw_step(None, None, None, None, 10, None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) == -1
    pd = ops.conv_pack_desc(8, 8, [8], [8])
    pd.Ktot += 64
    assert L.lib.uclstm_pack_weights(C.byref(pd), None, None, None) == -1
    with pytest.raises(L.UclstmError):
        L.check(-1, "x")


def test_fused_batchnorm_and_lstm_pointwise_contracts_are_checked_before_launch():
    """The shape contracts of the kernels tests/test_gpu_pointwise_abi.py calls directly: every pointer is non-null and 16-byte
    aligned (never dereferenced: nothing is launched), so UCLSTM_E_BADARG can only come from the shape."""
    P = C.c_void_p(1 << 20)
    for K in (L.lib, L.lib16):
        #                  n_img H  W  Cp    groups
        for geom in ((4, 5, 4, 8, 2),          # odd H
                     (4, 4, 7, 8, 2),          # odd W
                     (5, 4, 4, 8, 2),          # n_img % groups != 0
                     (4, 4, 4, 12, 2),         # Cp % 8 != 0
                     (4, 4, 4, 2056, 2)):      # Cp / 8 > 256: more chunk columns than threads
            assert K.uclstm_bn_apply_relu_pool(P, P, P, P, P, *geom, None) == -1, geom
            assert K.uclstm_bn_pool_bwd_reduce(P, P, P, P, P, P, P, P, P, *geom, None) == -1, geom
            assert K.uclstm_bn_pool_bwd_apply(P, P, P, P, P, P, P, P, P, *geom, None) == -1, geom
        #                  pixels ppg Cp   C
        for geom in ((100, 50, 24, 24),        # 3 lanes per pixel: not a power of two
                     (100, 50, 1024, 1024),    # 128 lanes: more than a wave
                     (100, 50, 64, 65),        # C > Cp
                     (100, 30, 64, 64)):       # pixels % pixels_per_group != 0
            assert K.uclstm_bn_head_fwd(P, P, P, P, P, P, *geom, None) == -1, geom
            assert K.uclstm_bn_head_bwd_reduce(P, P, P, P, P, P, P, P, P, P, P, *geom, None) == -1, geom
            assert K.uclstm_bn_head_bwd_apply(P, P, P, P, P, P, P, P, P, *geom, None) == -1, geom
        # f32 dh_b: at least one slab, and a slab stride of whole float4
        assert K.uclstm_lstm_bwd_pointwise(P, P, P, P, P, 1, 0, 0, P, 0, P, 10, 8, None) == -1
        assert K.uclstm_lstm_bwd_pointwise(P, P, P, P, P, 1, 3, 82, P, 0, P, 10, 8, None) == -1
        assert K.uclstm_lstm_bwd_pointwise(P, P, P, P, P, 2, 3, 82, P, 0, P, 10, 8, None) == -1
    for geom in ((4, 5, 4, 8, 2), (4, 4, 7, 8, 2), (5, 4, 4, 8, 2), (4, 4, 4, 12, 2), (4, 4, 4, 2056, 2)):
        assert L.lib.uclstm_bn_pool_bwd_rows(*geom) == -1, geom
    assert L.lib.uclstm_bn_pool_bwd_rows(4, 4, 4, 8, 2) == 2 and L.lib.uclstm_bn_pool_bwd_rows(2, 4, 4, 2048, 2) == 2


def test_pool_backward_block_plan_of_the_parity_shapes():
    """Rows of `partials` per group = min(ceil(windows per group / 32), max(1, 4096 // groups)) for every shape of the direct pool
    tests: the block boundaries those shapes are chosen for (a block ending inside an image, a ragged last block, the cap, empty
    trailing blocks) are really where the comments say."""
    from test_gpu_pointwise_abi import POOL_SHAPES
    for n_img, H, W, Cp, groups in POOL_SHAPES:
        wpg = (n_img // groups) * (H // 2) * (W // 2)
        rows = L.lib.uclstm_bn_pool_bwd_rows(n_img, H, W, Cp, groups)
        assert rows > 0 and rows % groups == 0, (n_img, H, W, Cp, groups)
        assert rows // groups == min(-(-wpg // 32), max(1, 4096 // groups)), (n_img, H, W, Cp, groups)
    plan = {s: L.lib.uclstm_bn_pool_bwd_rows(*s) // s[4] for s in POOL_SHAPES}
    assert plan[(4, 14, 6, 64, 2)] == 2 and plan[(2, 2, 66, 8, 1)] == 3 and plan[(1100, 20, 20, 8, 1100)] == 3
    assert plan[(2, 700, 400, 8, 1)] == 4096                  # 140000 windows: 4000 blocks of 35, the last 96 empty


def test_pack_descriptors_geometry():
    d = ops.conv_pack_desc(40, 24 + 8, [24, 8], [24, 8])
    assert (d.N, d.taps, d.kseg[0], d.kseg[1], d.Ktot) == (40, 9, 64, 64, 9 * 128)
    assert (d.choff[0], d.choff[1], d.stride_n, d.stride_k) == (0, 24, 32 * 9, 9)
    d = ops.lstm_pack_desc(1024, 1024)
    assert (d.N, d.Ktot, d.n_mode) == (4096, 9 * 2048, L.NMODE_LSTM)
    d = ops.lstm_pack_desc(5, 4)
    assert (d.N, d.kseg[0], d.kseg[1]) == (64, 64, 64)
    d = ops.lstm_dgrad_pack_desc(5, 4, 5)
    assert (d.N, d.kseg[0], d.k_hdp, d.k_hd, d.tap_flip) == (8, 64, 8, 5, 1)
    d = ops.lstm_wgrad_unpack_desc(1024, 1024)
    assert (d.N, d.Ktot, d.stride_ntap) == (4096, 9 * 2048, 1024 * 2048 * 9)
    d = ops.convt_pack_desc(1024, 512)
    assert (d.N, d.Ktot, d.n_cp, d.stride_n, d.stride_k, d.stride_ntap) == (2048, 1024, 512, 4, 2048, 1)
    d = ops.convt_dgrad_pack_desc(1024, 512)
    assert (d.N, d.taps, d.Ktot) == (1024, 4, 4 * 512)
    d = ops.im2col_pack_desc(64, 2, 24)
    assert (d.N, d.Ktot, d.k_mode, d.k_hd, d.k_hdp) == (64, 64, L.KMODE_IM2COL, 2, 9)


# ---------------------------------------------------------------------------------------------
# module surface
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [
    ("model_noskip", dict(base_ch=4, use_skip_lstm=False)),
    ("model_skip", dict(base_ch=4, use_skip_lstm=True)),
    ("model_2layer_att", dict(base_ch=2, lstm_layers=2, use_attention=True)),
])
def test_state_dict_keys_shapes_dtypes_equal_the_reference(name, kw):
    ref = sub(load_golden(name), "p/")
    m = U.TemporalUNetDualView(1, 1, **kw)
    sd = m.state_dict()
    assert list(sd.keys()) == sorted(sd.keys(), key=list(sd.keys()).index)       # deterministic
    assert set(sd.keys()) == set(ref.keys())
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape) and v.dtype == ref[k].dtype, k
    m.load_state_dict(ref, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ref[k]), k              # bit-exact round trip of the reference layout


def test_constructor_signatures_and_public_attributes():
    def params(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    assert params(U.ConvLSTMCell) == [("input_dim", inspect._empty), ("hidden_dim", inspect._empty), ("kernel_size", 3), ("bias", True)]
    assert params(U.ConvLSTM) == [("input_dim", inspect._empty), ("hidden_dim", inspect._empty), ("num_layers", 1), ("kernel_size", 3)]
    assert params(U.DoubleConv) == params(U.Down) == params(U.Up) == params(U.OutConv) == [("in_ch", inspect._empty), ("out_ch", inspect._empty)]
    assert params(U.SpatialAttention) == [("kernel_size", 7)]
    assert params(U.TemporalUNetDualView) == [("in_channels_per_sat", 1), ("out_channels", 1), ("base_ch", 32), ("lstm_layers", 1),
                                             ("use_skip_lstm", False), ("use_attention", False)]
    cell = U.ConvLSTMCell(3, 5)
    assert cell.hidden_dim == 5 and isinstance(cell.conv, torch.nn.Conv2d) and cell.conv.weight.shape == (20, 8, 3, 3)
    lstm = U.ConvLSTM(3, 5, num_layers=2)
    assert len(lstm.layers) == 2 and lstm.layers[1].conv.in_channels == 10
    m = U.TemporalUNetDualView(use_skip_lstm=True)
    assert m.use_skip_lstm and not m.use_attention and callable(m.encode_once) and U.UNet is U.TemporalUNetDualView
    up = U.Up(16, 8)
    assert up.up.weight.shape == (16, 8, 2, 2)


def test_same_seed_gives_the_reference_initialisation():
    """Parameter containers are stock torch modules created in the reference's order, so a seeded construction
    reproduces the reference's random init bit-for-bit (fixture 'model_skip' was built with seed 401)."""
    ref = sub(load_golden("model_skip"), "p/")
    torch.manual_seed(401)
    m = U.TemporalUNetDualView(1, 1, base_ch=4, lstm_layers=1, use_skip_lstm=True, use_attention=False)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_no_cpu_fallback():
    m = U.TemporalUNetDualView(base_ch=4)
    with pytest.raises(U.UclstmError):
        m(torch.rand(1, 2, 2, 16, 16))
    with pytest.raises(U.UclstmError):
        U.ConvLSTMCell(2, 4)(torch.rand(1, 2, 8, 8))
    with pytest.raises(U.UclstmError):
        U.compute_loss(torch.rand(1, 2, 1, 8, 8), torch.rand(1, 2, 1, 8, 8))
    with pytest.raises(RuntimeError):
        U.FusedAdamW([torch.nn.Parameter(torch.zeros(3))])


def test_npz_dataset_matches_reference_fixture(tmp_path):
    g = load_golden("dataset")
    path = tmp_path / "ds.npz"
    np.savez(path, X=g["X"].numpy(), Y=g["Y"].numpy())
    ds = U.NPZSequenceDataset(str(path))
    for k in ("norm_const", "min_vel", "max_vel", "y_scale", "trans_min", "trans_max"):
        assert abs(getattr(ds, k) - float(g[k])) <= 1e-6 * max(1.0, abs(float(g[k]))), k
    x, y, m = ds[1]
    torch.testing.assert_close(x, g["x1"])
    torch.testing.assert_close(y, g["y1"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(m, g["mask1"])
    torch.testing.assert_close(ds.denormalize(y).double(), g["denorm_y1"].double(), rtol=1e-5, atol=1e-5)
    assert len(ds) == 3


def test_synthetic_sequences_shapes_and_determinism():
    a = U.SyntheticSequences(2, 5, 32, 32, seed=3, kind="blobs", device="cpu")
    b = U.SyntheticSequences(2, 5, 32, 32, seed=3, kind="blobs", device="cpu")
    assert a.x.shape == (2, 5, 2, 32, 32) and a.y.shape == (2, 5, 1, 32, 32) and a.mask.shape == a.y.shape
    assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y)
    assert torch.equal(a.x[:, :, 0], a.x[:, :, 1])                       # frame duplicated into both views
    assert float(a.y.abs().max()) <= 1.0 and float(a.x.max()) <= 1.0
    u = U.SyntheticSequences(2, 3, 16, 16, seed=1, kind="uniform", device="cpu")
    assert 0.0 <= float(u.x.min()) and float(u.x.max()) < 1.0 and -1.0 <= float(u.y.min()) and float(u.y.max()) < 1.0


# ---------------------------------------------------------------------------------------------
# flat parameters + data-parallel gradient exchange (gloo, world_size 2)
# ---------------------------------------------------------------------------------------------
def test_flat_params_views_and_zero_grad():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    before = [p.detach().clone() for p in net.parameters()]
    fp = FlatParams(net.parameters())
    assert fp.numel == sum(p.numel() for p in net.parameters())
    for p, b, o in zip(net.parameters(), before, fp.offsets):
        assert torch.equal(p, b) and p.data_ptr() == fp.flat_p.data_ptr() + 4 * o
        assert p.grad.data_ptr() == fp.flat_g.data_ptr() + 4 * o
    net(torch.randn(4, 5)).sum().backward()
    assert float(fp.flat_g.abs().sum()) > 0
    for p, o in zip(net.parameters(), fp.offsets):                       # autograd accumulated IN PLACE into the flat buffer
        assert p.grad.data_ptr() == fp.flat_g.data_ptr() + 4 * o
    fp.zero_grad()
    assert float(fp.flat_g.abs().sum()) == 0


def _ddp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)                          # different init per rank: broadcast must fix it
    net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16), torch.nn.ReLU(), torch.nn.Linear(16, 2))
    net.register_buffer("stat", torch.full((3,), float(rank)))
    fp = FlatParams(net.parameters())
    ddp = FlatDDP(net, fp, bucket_mb=30 * 4 / (1 << 20))   # >= 30 floats per bucket -> three buckets
    p0 = fp.flat_p.clone()
    launched_during_backward = []
    orig = ddp._launch

    def spy(bi):
        launched_during_backward.append(bi)
        orig(bi)
    ddp._launch = spy
    torch.manual_seed(7 + rank)
    x = torch.randn(8, 6)
    fp.zero_grad()
    ddp.reset()
    net(x).pow(2).mean().backward()
    n_early = len(launched_during_backward)
    ddp.finalize()
    # numpy copies: pickled by value (torch tensors would travel as shared-memory handles that die with this process)
    q.put((rank, p0.numpy().copy(), fp.flat_g.numpy().copy(), x.numpy().copy(), n_early, len(ddp.buckets), net.stat.numpy().copy()))
    dist.destroy_process_group()


def test_flat_ddp_two_ranks_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res = [tuple(torch.from_numpy(v) if isinstance(v, np.ndarray) else v for v in r) for r in res]
    (_, p_a, g_a, x_a, early_a, nb, stat_a), (_, p_b, g_b, x_b, early_b, _, stat_b) = res
    assert torch.equal(p_a, p_b)                           # parameters broadcast from rank 0
    assert torch.equal(stat_a, stat_b) and float(stat_a[0]) == 0.0      # buffers too
    assert torch.equal(g_a, g_b)                           # every rank holds the same averaged gradient
    assert nb >= 3 and early_a == nb and early_b == nb     # every bucket was launched from a backward hook (overlap)
    # reference: mean of the two ranks' local gradients
    net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16), torch.nn.ReLU(), torch.nn.Linear(16, 2))
    fp = FlatParams(net.parameters())
    fp.flat_p.copy_(p_a)
    gs = []
    for x in (x_a, x_b):
        fp.zero_grad()
        net(x).pow(2).mean().backward()
        gs.append(fp.flat_g.clone())
    torch.testing.assert_close(g_a, (gs[0] + gs[1]) / 2, rtol=1e-6, atol=1e-7)


def _ddp_bf16_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.ReLU(), torch.nn.Linear(16, 2))
    fp = FlatParams(net.parameters())
    ddp = FlatDDP(net, fp, bucket_mb=30 * 4 / (1 << 20), grad_dtype=torch.bfloat16)
    torch.manual_seed(7 + rank)
    x = torch.randn(8, 6)
    fp.zero_grad()
    ddp.reset()
    net(x).pow(2).mean().backward()
    local = fp.flat_g.clone()
    ddp.finalize()
    q.put((rank, local.numpy().copy(), fp.flat_g.numpy().copy()))
    dist.destroy_process_group()


def test_flat_ddp_bf16_buckets_two_ranks_gloo():
    """grad_dtype=bfloat16: every bucket is exchanged as bf16 (half the bytes), result = mean of the bf16-rounded local
    gradients, identical on both ranks, back in the f32 gradient buffer."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_ddp_bf16_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, la, ga), (_, lb, gb) = [tuple(torch.from_numpy(v) if isinstance(v, np.ndarray) else v for v in r) for r in res]
    assert torch.equal(ga, gb)
    want = ((la.bfloat16() + lb.bfloat16()).float() / 2)            # gloo sums in bf16, the mean is taken in f32
    torch.testing.assert_close(ga, want, rtol=1e-2, atol=1e-6)
    exact = (la + lb) / 2
    assert float((ga - exact).norm() / exact.norm()) <= 1e-2        # bf16 exchange: <= 2^-8 relative per element


def test_flat_ddp_counts_uses_of_side_written_gradients():
    """A parameter whose gradient is written by the operators themselves announces once per USE: the bucket may only be
    released after as many announcements as the forward pass reported uses (a module called twice under one backward),
    and ``no_sync()`` passes neither count nor launch."""
    if dist.is_initialized():
        dist.destroy_process_group()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(33500 + (os.getpid() % 2000))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        net = torch.nn.Linear(4, 3)
        fp = FlatParams(net.parameters())
        ddp = FlatDDP(net, fp, bucket_mb=1.0, first_bucket_mb=1e-9)
        launched = []
        orig = ddp._launch
        ddp._launch = lambda bi: (launched.append(bi), orig(bi))[1]
        w, b = net.weight, net.bias
        iw, ib = ddp._index_of[id(w)], ddp._index_of[id(b)]
        fp.zero_grad()
        ddp.reset()
        U.ops.note_use(w)
        U.ops.note_use(w)                                  # the module ran twice before backward
        U.ops.grad_written(w)
        assert not launched and not ddp._done[iw]          # first announcement of two: nothing may start
        U.ops.grad_written(w)
        assert ddp._done[iw]
        ddp._on_ready(ib)                                  # autograd's accumulator: once per backward, completes at once
        assert sorted(launched) == list(range(len(ddp.buckets)))
        ddp.finalize()
        with pytest.raises(RuntimeError, match="announced 3 gradients for 2 recorded uses"):
            U.ops.grad_written(w)                          # a third announcement for two uses is a protocol error
        # gradient accumulation: passes inside no_sync() are invisible
        launched.clear()
        ddp.reset()
        with ddp.no_sync():
            U.ops.note_use(w)
            U.ops.grad_written(w)
            ddp._on_ready(ib)
        assert not launched and ddp._uses[iw] == 0
        U.ops.note_use(w)
        U.ops.grad_written(w)
        ddp._on_ready(ib)
        assert sorted(launched) == list(range(len(ddp.buckets)))
        ddp.finalize()
        # a forward inside no_sync() whose backward runs outside (or a forward before reset()): the number of uses of this
        # pass is unknown, so a side announcement must NOT release the bucket on the first of T per-timestep gradients --
        # it is left to finalize() (uses 0 -> expected max(1, 0) = 1 released early, then asserted)
        launched.clear()
        ddp.reset()
        with ddp.no_sync():
            U.ops.note_use(w)
            U.ops.note_use(w)
        U.ops.grad_written(w)
        U.ops.grad_written(w)
        assert not launched and not ddp._done[iw]
        ddp.reset()
        U.ops.grad_written(w)                              # gradient of a forward that ran before reset(): never early
        assert not launched and not ddp._done[iw]
        ddp.finalize()
        assert sorted(launched) == list(range(len(ddp.buckets)))
        # one gradient buffer, one wrapper
        with pytest.raises(RuntimeError, match="already belong"):
            FlatDDP(net, fp)
        ddp.remove_hooks()
        assert not U.ops.USE_HOOKS and not U.ops.GRAD_SIDE_HOOKS
        # a wrapper dropped WITHOUT remove_hooks() takes its global hooks with it
        d2 = FlatDDP(net, fp)
        assert len(U.ops.USE_HOOKS) == 1 and len(U.ops.GRAD_SIDE_HOOKS) == 1
        for h in d2._hooks:
            h.remove()
        d2._hooks = []
        del d2
        import gc
        gc.collect()
        assert not U.ops.USE_HOOKS and not U.ops.GRAD_SIDE_HOOKS
        d3 = FlatDDP(net, fp)
        assert d3.describe() == {"buckets": len(d3.buckets), "allreduce_bytes": 4 * fp.numel, "dtype": "f32", "world_size": 1,
                                 "bucket_bytes": [4 * (hi - lo) for lo, hi in d3.ranges]}
        d3.remove_hooks()
    finally:
        dist.destroy_process_group()


def test_bench_self_launch_starts_n_ranks():
    """``python bench.py --gpus 2`` without torchrun must start two ranks itself (the driver's N>1 invocation) -- checked
    with --dry-launch, which rendezvouses over gloo on the CPU and reports what every rank saw."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["dry_launch"] and out["n_gpus"] == 2
    assert sorted(x["rank"] for x in out["ranks"]) == [0, 1] and all(x["world_size"] == 2 for x in out["ranks"])
    assert out["scaling"] == "weak" and all(x["per_gpu_batch"] == 32 for x in out["ranks"]) and out["global_batch"] == 64
    # strong scaling: the global batch is fixed and divided over the ranks
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch", "--scaling", "strong", "--global-batch", "32"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["scaling"] == "strong" and out["global_batch"] == 32 and all(x["per_gpu_batch"] == 16 for x in out["ranks"])
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch", "--scaling", "strong", "--global-batch", "33"],
                       env={**env, "RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0"}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "multiple" in (r.stderr + r.stdout)
    # the launcher parent never loads torch (a process that starts GPU programs makes no GPU call, not even a device count)
    probe = ("import sys, runpy; sys.argv=['bench.py','--gpus','2','--dry-launch'];\n"
             "import subprocess; subprocess.run=lambda *a, **k: type('R', (), {'returncode': 0})()\n"
             "try:\n    runpy.run_path(%r, run_name='__main__')\nexcept SystemExit: pass\n"
             "print('TORCH_LOADED' if 'torch' in sys.modules else 'TORCH_ABSENT')" % os.path.join(root, "bench.py"))
    r = subprocess.run([sys.executable, "-c", probe], env=env, capture_output=True, text=True, timeout=120)
    assert "TORCH_ABSENT" in r.stdout, (r.stdout, r.stderr[-1000:])
    # a rank count that does not match --gpus is refused, never silently run as one rank
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch"],
                       env={**env, "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_launch_plan_splits_tensors_beyond_the_descriptor_range():
    """A single GEMM launch addresses < 2 GiB per tensor (bit 31 of a buffer offset = outside).  The reference's own
    256x256 setting (B=32, T=8, base_ch=64: 2^31 bytes in the inc / up0 layers) must be cut into image ranges on
    BatchNorm-group boundaries instead of failing with 'bad argument'."""
    ops = U.ops
    per_img = 256 * 256 * 64 * 2
    n_img, groups = 8 * 32, 8
    assert n_img * per_img == 1 << 31
    ch = ops._img_chunks(n_img, groups, per_img, "t", whole_groups=True)
    assert len(ch) >= 2 and ch[0][0] == 0 and ch[-1][1] == n_img
    for (a, b), (c, _) in zip(ch, ch[1:] + [(n_img, n_img)]):
        assert b == c and (b - a) % (n_img // groups) == 0 and (b - a) * per_img < ops.LAUNCH_BYTES_LIMIT
    assert ops._img_chunks(48, 12, 256 * 256 * 64 * 2, "t", whole_groups=True) == [(0, 48)]        # config 4 (B=4, T=12) fits
    free = ops._img_chunks(n_img, 1, per_img, "t")
    assert all((b - a) * per_img < ops.LAUNCH_BYTES_LIMIT for a, b in free) and free[-1][1] == n_img
    with pytest.raises(U.UclstmError, match="exceeds"):
        ops._img_chunks(2, 2, 1 << 31, "t", whole_groups=True)


def test_panel_cache_is_owned_and_invalidated_by_weight_updates():
    ops = U.ops
    c = ops.PanelCache()
    assert not c.stale() and ops._ACTIVE_CACHE is None
    with c:
        assert ops._ACTIVE_CACHE is c
    assert ops._ACTIVE_CACHE is None
    ops.weights_changed()                                  # what FusedAdamW.step() does
    assert c.stale() and not ops.PanelCache().stale()
    c.clear()
    assert not c.stale()
    assert not hasattr(ops, "_PANEL_CACHE")                # no module-global cache any more


def test_pack_job_table_families_and_segments():
    """Host side of the batched look-ahead packing: uclstm_pack_job_init (a host function) classifies a panel into its kernel
    family and sizes its block range as the single-panel launch would; ops.pack_segments cuts the panels into segments at
    cumulative byte fractions."""
    import ctypes as C
    cases = [(ops.conv_pack_desc(72, 80, [56, 24], [56, 24]), 1, (1 + 1) * 72),               # rows, 9 taps: (chunks0 + chunks1) x N
             (ops.lstm_pack_desc(40, 24), 1, None),
             (ops.convt_dgrad_pack_desc(48, 24), 2, None),                                    # rows, 4 taps
             (ops.conv_dgrad_pack_desc(200, 136, 136), 3, ((200 + 63) // 64) * ((136 + 15) // 16)),   # transposed: 64 K columns x 16 rows
             (ops.lstm_dgrad_pack_desc(40, 24, 40), 3, None),
             (ops.convt_pack_desc(48, 24), 0, None)]                                          # generic
    w = (C.c_float * 4)()
    for d, family, nblocks in cases:
        job = L.PackJob()
        rc = L.lib.uclstm_pack_job_init(C.byref(job), C.byref(d), C.cast(w, C.c_void_p), C.cast(w, C.c_void_p), 5)
        assert rc == family == job.family, (rc, family)
        assert job.block0 == 5 and job.nblocks >= 1 and job.gx >= 1 and job.nblocks % job.gx == 0
        if nblocks is not None:
            assert job.nblocks == nblocks, (job.nblocks, nblocks)
        assert bytes(job.d) == bytes(d) and job.div[2] == d.Ktot
    assert L.lib.uclstm_pack_job_init(None, C.byref(cases[0][0]), C.cast(w, C.c_void_p), C.cast(w, C.c_void_p), 0) == -1
    assert L.lib.uclstm_pack_job_init(C.byref(L.PackJob()), C.byref(cases[0][0]), None, C.cast(w, C.c_void_p), 0) == -1
    sizes = [1, 1, 8, 10, 30, 50]
    assert ops.pack_segments(sizes, (0.02, 0.2, 0.5)) == [0, 0, 1, 1, 2, 3]
    assert ops.pack_segments(sizes, ()) == [0] * 6
    seg = ops.pack_segments([7] * 40, ops.PACK_SEGMENTS)
    assert seg[0] == 0 and seg == sorted(seg) and seg[-1] == len(ops.PACK_SEGMENTS)


def test_store_split_k_long_k_rule_is_off_by_default_and_narrow_when_on(monkeypatch):
    """ops.store_split_k: K ranges of a statistics-free store convolution.  The long-K rule is OFF by default: alone it makes one launch
    of the headline step 23 % faster, in the overlapped step the backward phase does not gain (profiles/round3_store_splitk*.txt).
    Switched on (288 K-steps) it must pick 2 ranges only for the two measured winners and leave every shape that LOST alone."""
    assert ops.SPLITK_STORE_LONGK_STEPS == 0 or "UCLSTM_SPLITK_STORE_LONGK" in os.environ
    monkeypatch.setattr(ops, "SPLITK_STORE_LONGK_STEPS", 0)
    assert ops.store_split_k(640 * 16, 1024, 36864 // 64) == 1
    monkeypatch.setattr(ops, "SPLITK_STORE_LONGK_STEPS", 288)
    assert ops.store_split_k(640 * 16, 1024, 36864 // 64) == 2                       # temporal ConvLSTM input gradient, 64 x 64 seq-20 B=32
    assert ops.store_split_k(48 * 256, 1024, 36864 // 64) == 2                        # the same layer at 256 x 256 seq-12 B=4: 384 tiles, measured
    lost = [(640 * 64, 512, 4608), (640 * 16, 1024, 9216), (640 * 64, 512, 18432), (640 * 16, 1024, 4608), (640 * 16, 512, 9216),
            (640 * 64, 256, 4608), (640 * 64, 512, 2304), (640 * 256, 256, 2304)]
    for pixels, N, K in lost:
        assert ops.store_split_k(pixels, N, K // 64) == 1, (pixels, N, K)
    assert ops.store_split_k(256 * 64, 1024, 36864 // 64) == 1                        # 128 x 128 seq-8 B=32: 512 tiles = two exact rounds
    assert ops.store_split_k(1 * 16 * 16, 256, 2304 // 64) > 1                         # the old small-grid rule (batch-1 inference) still applies


# ---------------------------------------------------------------------------------------------
# the f64 reference, the dispatch plan and the argument contracts of tests/test_gpu_igemm_abi.py
# ---------------------------------------------------------------------------------------------
def _ref_conv(n_img, H, W, ktap, scale, pad, srcs, w, cs, N):
    """tests/igemm_cases.py reference on NHWC f64 sources with a host-written panel -> [n_img][N][H][W]."""
    import igemm_cases as IC
    A = IC.gather_a(n_img, H, W, ktap, scale, pad, [(x.permute(0, 2, 3, 1).contiguous(), oy, ox) for x, oy, ox in srcs])
    out, mag = IC.gemm_ref(A, IC.host_panel(w, cs, ktap, N))
    assert bool((mag >= out.abs() - 1e-12).all())
    return out.view(n_img, H, W, N).permute(0, 3, 1, 2)


def test_igemm_f64_reference_equals_pytorch_convolutions():
    """The host reference of the direct forward-GEMM tests against f64 F.conv2d / F.conv_transpose2d / F.pad: 3x3, two sources with
    positive (pad) and negative (crop) offsets, 1x1, 5x5 / 7x7 on images smaller than the kernel, the ConvTranspose forward
    segments (also onto a larger and a smaller destination) and the scale-2 gather with an even and an odd source."""
    import torch.nn.functional as F
    import igemm_cases as IC
    torch.manual_seed(5)
    dd = torch.float64
    n, H, W = 3, 9, 11
    x0 = torch.randn(n, 24, H, W, dtype=dd)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    w = torch.randn(37, 24, 3, 3, dtype=dd)
    close(_ref_conv(n, H, W, 3, 1, 1, [(x0, 0, 0)], w, [24], 40)[:, :37], F.conv2d(x0, w, padding=1))
    assert bool((_ref_conv(n, H, W, 3, 1, 1, [(x0, 0, 0)], w, [24], 40)[:, 37:] == 0).all())
    # second source smaller, placed at (1, 1): F.pad left/top 1, right 1, bottom 2 (train/unet.py:95-98)
    w2 = torch.randn(37, 40, 3, 3, dtype=dd)
    u = torch.randn(n, 16, H - 3, W - 2, dtype=dd)
    close(_ref_conv(n, H, W, 3, 1, 1, [(x0, 0, 0), (u, 1, 1)], w2, [24, 16], 40)[:, :37],
          F.conv2d(torch.cat((x0, F.pad(u, [1, 1, 1, 2])), 1), w2, padding=1))
    # second source larger, offsets (-1, -2): the window [1, 1 + H) x [2, 2 + W) of it lies on the grid.  The header's rule is
    # "zero outside [0, Hs) x [0, Ws)", so border taps read the source's real pixels around that window (a crop followed by a padded
    # convolution would see zeros there): an unpadded convolution over the window grown by one pixel
    u = torch.randn(n, 16, H + 2, W + 3, dtype=dd)
    close(_ref_conv(n, H, W, 3, 1, 1, [(x0, 0, 0), (u, -1, -2)], w2, [24, 16], 40)[:, :37],
          F.conv2d(x0, w2[:, :24], padding=1) + F.conv2d(u[:, :, 0:H + 2, 1:W + 3], w2[:, 24:]))
    u = torch.randn(n, 16, H + 1, W + 2, dtype=dd)          # window flush with the source's bottom / right edge: zeros beyond it
    close(_ref_conv(n, H, W, 3, 1, 1, [(x0, 0, 0), (u, -1, -2)], w2, [24, 16], 40)[:, :37],
          F.conv2d(x0, w2[:, :24], padding=1) + F.conv2d(F.pad(u, [0, 1, 0, 1])[:, :, 0:H + 2, 1:W + 3], w2[:, 24:]))
    # 1x1 over a 72-channel source (two K chunks, the second 8 of 64)
    x1 = torch.randn(n, 72, H, W, dtype=dd)
    w1 = torch.randn(13, 72, 1, 1, dtype=dd)
    close(_ref_conv(n, H, W, 1, 1, 0, [(x1, 0, 0)], w1, [72], 16)[:, :13], F.conv2d(x1, w1))
    # 5x5 / 7x7, also on 3x4 images
    for k in (5, 7):
        for h, wd in ((9, 11), (3, 4)):
            xs = torch.randn(n, 16, h, wd, dtype=dd)
            wk = torch.randn(21, 16, k, k, dtype=dd)
            close(_ref_conv(n, h, wd, k, 1, k // 2, [(xs, 0, 0)], wk, [16], 24)[:, :21], F.conv2d(xs, wk, padding=k // 2))
    # scale-2 gather (ConvTranspose2d(k2, s2) input gradient = stride-2 2x2 convolution), even and odd source
    h, wd = 5, 6
    wg = torch.randn(37, 24, 2, 2, dtype=dd)
    xs = torch.randn(n, 24, 2 * h, 2 * wd, dtype=dd)
    close(_ref_conv(n, h, wd, 2, 2, 0, [(xs, 0, 0)], wg, [24], 40)[:, :37], F.conv2d(xs, wg, stride=2))
    xs = torch.randn(n, 24, 2 * h - 1, 2 * wd - 1, dtype=dd)
    close(_ref_conv(n, h, wd, 2, 2, 0, [(xs, 0, 0)], wg, [24], 40)[:, :37], F.conv2d(F.pad(xs, [0, 1, 0, 1]), wg, stride=2))
    # ConvTranspose2d forward: 1x1 GEMM with tap-major rows n = tap*Cop + co, four scale-2 segments
    Co, Cop = 13, 16
    xs = torch.randn(n, 24, h, wd, dtype=dd)
    wt = torch.randn(24, Co, 2, 2, dtype=dd)
    wp = torch.zeros(4 * Cop, 64, dtype=dd)
    for t in range(4):
        wp[t * Cop:t * Cop + Co, :24] = wt[:, :, t // 2, t % 2].t()
    A = IC.gather_a(n, h, wd, 1, 1, 0, [(xs.permute(0, 2, 3, 1).contiguous(), 0, 0)])
    val, _ = IC.gemm_ref(A, wp)
    full = F.conv_transpose2d(xs, wt, stride=2)
    for Hd, Wd in ((2 * h, 2 * wd), (2 * h + 1, 2 * wd + 1), (2 * h - 1, 2 * wd - 1)):
        segs = [(t * Cop, (t + 1) * Cop, Cop, 0, Hd, Wd, 2, t // 2, t % 2) for t in range(4)]
        dsts = IC.scatter_segments(val, n, h, wd, segs)
        merged = torch.full((n, Hd, Wd, Cop), float("nan"), dtype=dd)
        for dst in dsts:
            assert not bool((~torch.isnan(dst) & ~torch.isnan(merged)).any())       # the four taps never collide
            merged = torch.where(torch.isnan(dst), merged, dst)
        hh, ww = min(Hd, 2 * h), min(Wd, 2 * wd)
        close(merged[:, :hh, :ww, :Co].permute(0, 3, 1, 2), full[:, :, :hh, :ww])
        assert bool(torch.isnan(merged[:, 2 * h:]).all()) and bool(torch.isnan(merged[:, :, 2 * wd:]).all())
        assert not bool(torch.isnan(merged[:, :hh, :ww]).any())
    # c_off into a wider destination and a column range: everything else stays unwritten
    dst = IC.scatter_segments(val, n, h, wd, [(8, 32, 48, 16, h, wd, 1, 0, 0)])[0]
    close(dst[..., 16:40].reshape(-1, 24), val[:, 8:32])
    assert bool(torch.isnan(dst[..., :16]).all()) and bool(torch.isnan(dst[..., 40:]).all())
    # K ranges: the partial sums add up to the full sum, range r holds the chunks [r*cpr, (r+1)*cpr) of every tap
    A = IC.gather_a(n, H, W, 3, 1, 1, [(x1.permute(0, 2, 3, 1).contiguous(), 0, 0), (x0.permute(0, 2, 3, 1).contiguous(), 0, 0)])
    wp = torch.randn(8, 9 * 192, dtype=dd)
    for ks, sizes in ((1, [3]), (2, [2, 1]), (8, [1, 1, 1])):
        masks = IC.krange_masks(3, [128, 64], ks)
        assert [int(m.sum()) // (9 * 64) for m in masks] == sizes and len(masks) == L.lib.uclstm_igemm_ksplit_used(9 * 192, 3, ks)
        close(sum(IC.gemm_ref(A, wp, m)[0] for m in masks), IC.gemm_ref(A, wp)[0])
    assert [int(m.sum()) // (9 * 64) for m in IC.krange_masks(3, [320], 3)] == [2, 2, 1]
    # the cell: gate order and row interleave (n = hb*64 + gate*16 + j), against torch.chunk on the reference's channel order
    pre = torch.randn(7, 128, dtype=dd)
    g = IC.lstm_rows_to_gates(pre, 24)
    assert g.shape == (7, 4, 24) and float(g[3, 2, 17]) == float(pre[3, 64 + 2 * 16 + 1])
    cp = torch.randn(7, 24, dtype=dd)
    gates, cn, hn = IC.lstm_cell_ref(g, cp)
    i, f, gg, o = torch.chunk(g.reshape(7, 96), 4, dim=1)
    close(cn, torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(gg))
    close(hn, torch.sigmoid(o) * torch.tanh(cn))


def test_igemm_parity_cases_dispatch_plan():
    """Every case of tests/test_gpu_igemm_abi.py really reaches the kernel, tile count and K-range count it is meant for
    (validation-only entry points, dummy aligned pointers)."""
    import igemm_cases as IC
    names = [c.name for c in IC.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in IC.ALL_CASES + IC.GROUP_B:
        d = IC.dummy_desc(c)
        assert L.lib.uclstm_igemm_fwd_shape(C.byref(d)) == c.shape, c.name
        if c.stats:
            tiles = IC.stats_tiles(c)
            assert len(tiles) == c.groups * L.lib.uclstm_igemm_tiles_per_group(c.n_img, c.H, c.W, c.groups, c.N), c.name
            assert max(len(p) for p in tiles) == min(c.tile_pixels(), c.M // c.groups)
    plan = {c.name: c for c in IC.ALL_CASES}
    tpg = lambda c: L.lib.uclstm_igemm_tiles_per_group(c.n_img, c.H, c.W, c.groups, c.N)
    assert [tpg(plan[k]) for k in ("S9-k0-g3", "S9-k1-g3", "S9-k0-g2", "S9-k1-g2")] == [1, 1, 3, 2]      # 99 and 384 pixels per group
    assert [tpg(plan[k]) for k in ("S11-a", "S11-b", "S11-c", "S12-a", "S12-b", "S13-b", "S13-c")] == [2, 2, 6, 4, 12, 4, 5]
    # the ring case above 256 tiles: 129 blocks of two tiles and one of one; three group boundaries cut a block's run
    runs = IC.stats_runs(plan["S13-e"])
    assert tpg(plan["S13-e"]) == 37 and len(runs) == 133 and sum(len(r[0]) for r in runs) == 126
    assert all(len(r[0]) == 0 for r in IC.stats_runs(plan["S13-b"]))
    # every kernel and epilogue is reached
    assert {(c.epi, c.shape) for c in IC.ALL_CASES} >= {(L.EPI_STORE, 0), (L.EPI_STORE, 1), (L.EPI_STORE, 2), (L.EPI_STORE, 3),
                                                         (L.EPI_ATOMIC, 0), (L.EPI_ATOMIC, 1), (L.EPI_ATOMIC, 2), (L.EPI_LSTM, 0), (L.EPI_LSTM, 2)}
    for c in IC.ATOMIC_CASES:
        assert L.lib.uclstm_igemm_ksplit_used(c.Ktot, c.ktap, c.ksplit) == IC.ATOMIC_USED[c.name.split("-")[-1]], c.name
    for members in (IC.GROUP_A, IC.GROUP_B):
        arr = (L.IgemmDesc * len(members))(*[IC.dummy_desc(c) for c in members])
        assert L.lib.uclstm_igemm_fwd_group_blocks(arr, len(members)) == IC.group_blocks_expected(members)
    assert IC.group_blocks_expected(IC.GROUP_A) == 24 and IC.group_blocks_expected(IC.GROUP_B) == 40


def test_igemm_forward_contracts_are_checked_before_launch():
    """UCLSTM_E_BADARG of the forward family beyond test_argument_contracts_are_checked_before_launch; every descriptor below is a
    valid case of the parity table with ONE field broken (the unbroken one is accepted first)."""
    import igemm_cases as IC
    plan = {c.name: c for c in IC.ALL_CASES}
    shape = lambda d: L.lib.uclstm_igemm_fwd_shape(C.byref(d))
    # split-K: acc_ld < N, a slab smaller than the output
    c = plan["A-k0-s2"]
    d = IC.dummy_desc(c)
    assert shape(d) == 0
    d.acc_ld = c.N - 8
    assert shape(d) == -1
    d = IC.dummy_desc(c)
    d.acc_slab = c.M * d.acc_ld - 1
    assert shape(d) == -1
    d = IC.dummy_desc(c)
    d.ksplit = 0
    assert shape(d) == -1
    # stats with a kernel wider than 3x3
    c = plan["S10-5"]
    d = IC.dummy_desc(c)
    assert shape(d) == 0
    d.stats = IC.DUMMY
    assert shape(d) == -1
    # a segment that does not fit its destination's channels
    c = plan["S7"]
    d = IC.dummy_desc(c)
    assert shape(d) == 0
    d.seg[0].c_off = 32                 # 32 + 24 > 48
    assert shape(d) == -1
    # fused cell: misaligned pre_add, N != 64 * ceil(Hd_p / 16)
    c = plan["L0-hd24"]
    d = IC.dummy_desc(c)
    assert shape(d) == 0
    d.pre_add = IC.DUMMY + 4
    assert shape(d) == -1
    d = IC.dummy_desc(c)
    d.Hd_p = 40                         # needs N = 192
    assert shape(d) == -1
    d = IC.dummy_desc(c)
    d.c_out = None
    assert shape(d) == -1
    # group launch: a member that is not on the patch shape, mixed source counts
    ok = [IC.dummy_desc(m) for m in IC.GROUP_A]
    blocks = lambda ds: L.lib.uclstm_igemm_fwd_group_blocks((L.IgemmDesc * len(ds))(*ds), len(ds))
    assert blocks(ok) == 24
    assert blocks(ok + [IC.dummy_desc(plan["A-k0-s2"])]) == -1          # per-tap shape
    assert blocks(ok + [IC.dummy_desc(plan["S8-k2"])]) == -1            # patch shape, STORE epilogue
    assert blocks(ok + [IC.dummy_desc(plan["L2-h-only"])]) == -1        # one source among two-source members
    assert blocks([IC.dummy_desc(plan["L2-h-only"])]) == 8
    assert blocks(ok * 2) == -1                                          # more than four members
    for K in (L.lib, L.lib16):
        assert K.uclstm_igemm_fwd_group((L.IgemmDesc * 4)(*(ok + [IC.dummy_desc(plan["A-k0-s2"])])), 4, None) == -1


# ---------------------------------------------------------------------------------------------
# the f64 reference, the dispatch plan and the argument contracts of tests/test_gpu_wgrad_abi.py
# ---------------------------------------------------------------------------------------------
def _autograd_panel(c, xs, dys):
    """f64 weight-gradient panel [N][Ktot] of a tests/wgrad_cases.py case from torch autograd on sum(op(x, w) * dy), placed with
    igemm_cases.host_panel.  Sources are put on the pixel frame with F.pad (a negative pad crops); dY comes from plain slices."""
    import torch.nn.functional as F
    import igemm_cases as IC
    nchw = lambda t: t.permute(0, 3, 1, 2)
    if c.kind == "convt":
        x, du = nchw(xs[0]), nchw(dys[0])
        Ci, Cop = x.shape[1], du.shape[1]
        w = torch.zeros(Ci, Cop, 2, 2, dtype=torch.float64, requires_grad=True)
        (F.conv_transpose2d(x, w, stride=2) * du).sum().backward()
        return IC.host_panel(w.grad.permute(2, 3, 1, 0).reshape(4 * Cop, Ci, 1, 1), [Ci], 1, c.N)       # row (ty*2 + tx)*Cop + co
    hh, ww = (c.H - 1) * c.scale + c.ktap, (c.W - 1) * c.scale + c.ktap       # frame rows / columns -pad ... that the taps reach
    frame = []
    for x, (_, Hs, Ws, offY, offX) in zip(xs, c.srcs):
        top, left = c.pad + offY, c.pad + offX
        frame.append(F.pad(nchw(x), [left, ww - left - Ws, top, hh - top - Hs]))
    dy = torch.zeros(c.n_img, c.N, c.H, c.W, dtype=torch.float64)
    for n0, n1, ti, c_off, sc, oy, ox in c.segments():
        assert (sc, oy, ox) == (1, 0, 0)
        dy[:, n0:n1] = nchw(dys[ti])[:, c_off:c_off + n1 - n0]
    cs = [s[0] for s in c.srcs]
    w = torch.zeros(c.N, sum(cs), c.ktap, c.ktap, dtype=torch.float64, requires_grad=True)
    (F.conv2d(torch.cat(frame, 1), w, stride=c.scale) * dy).sum().backward()
    return IC.host_panel(w.grad, cs, c.ktap, c.N)


def test_wgrad_f64_reference_equals_pytorch_autograd():
    """The host reference of the direct weight-gradient tests against f64 autograd: 3x3 with one and two sources, padded (F.pad)
    and cropped second source, ConvTranspose2d (four scale-2 dY segments, also with a row tile that spans segments), 5x5 / 7x7,
    the scale-2 gather, dY as channel slices of wider tensors with uncovered rows, two segments, the gate convolution over
    cat(x, h), 1x1 and an image smaller than a stage.  Valid elements agree to 1e-12; padding elements are exactly 0."""
    import igemm_cases as IC
    import wgrad_cases as WC
    for name in WC.AUTOGRAD_CASES:
        c = WC.case(name)
        xs, dys = WC.make_operands(c, torch.float64)
        ref, mag = WC.case_ref(c, xs, dys)
        want = _autograd_panel(c, xs, dys)
        assert ref.shape == want.shape == (c.N, c.Ktot), name
        # padding: K columns beyond a source's channels, rows that no segment covers
        valid = IC.host_panel(torch.ones(c.N, sum(s[0] for s in c.srcs), c.ktap, c.ktap, dtype=torch.float64), [s[0] for s in c.srcs],
                              c.ktap, c.N) != 0
        covered = torch.zeros(c.N, dtype=torch.bool)
        for n0, n1, *_ in c.segments():
            covered[n0:n1] = True
        valid &= covered[:, None]
        assert int(valid.sum()) == sum(n1 - n0 for n0, n1, *_ in c.segments()) * c.ktap ** 2 * sum(s[0] for s in c.srcs), name
        assert bool((ref[~valid] == 0).all()) and bool((mag[~valid] == 0).all()) and bool((want[~valid] == 0).all()), name
        assert bool((mag[valid] > 0).all()) and bool((mag >= ref.abs() * (1 - 1e-12)).all()), name
        torch.testing.assert_close(ref[valid], want[valid], rtol=1e-12, atol=1e-12, msg=lambda m: f"{name}: {m}")


def test_wgrad_parity_cases_dispatch_plan_and_rejected_descriptors():
    """Every case of tests/test_gpu_wgrad_abi.py reaches the kernel it is meant for (validation-only entry points, dummy aligned
    pointers), both tiles of the C_out <= 64 kernel are taken, and the broken descriptors are refused by the query."""
    import wgrad_cases as WC
    names = [c.name for c in WC.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in WC.ALL_CASES:
        d = WC.build_wgrad_desc(c)
        assert WC.wgrad_shape(d) == c.shape, c.name
        assert WC.wgrad_splits(d) >= 1, c.name
        assert c.M * c.N * c.Ktot <= 4e9, c.name
    assert {c.shape for c in WC.ALL_CASES} == {0, 1, 2, 3, 4}
    assert set(WC.MODE_CASES) == {0, 1, 2, 3} and all(WC.case(n).shape == k for k, n in WC.MODE_CASES.items())
    # 64 x 192 when 192 | Ktot (every 3x3 gradient: Ktot = 576 * chunks), else 64 x 256
    assert {c.name: c.Ktot % 192 == 0 for c in WC.P64_CASES} == {
        "W1-576": True, "W1-two-1152": True, "W1-two-k1-128": False, "W1-c64": True, "W1-k1": False, "W1-small-image": True,
        "W1-lstm16": True}
    # generic addressing: both instantiations (PLAIN = every operand dense on the output grid)
    plain = lambda c: c.scale == 1 and all(s[1:] == (c.H, c.W, 0, 0) for s in c.srcs) and \
        all(t[1:] == (c.H, c.W) for t in c.dy_tensors()) and all(s[4:] == (1, 0, 0) for s in c.segments())
    assert {plain(c) for c in WC.GENERIC_CASES} == {True, False}
    # the ring kernel needs slab mode: with slab = 0 the same descriptor goes where the case says
    for c in WC.RING_CASES:
        assert WC.wgrad_shape(WC.build_wgrad_desc(c, slab=0)) == c.atomic_shape != 4, c.name
        grid = WC.wgrad_splits(WC.build_wgrad_desc(c))
        assert WC.wgrad_splits(WC.build_wgrad_desc(c, splits=grid + 1)) == grid
    # the power-of-two image with two dY segments would be a fast-path case with one
    c = WC.case("W0-pow2-nseg2")
    d = WC.build_wgrad_desc(c)
    d.nseg, d.seg[0].n_end, d.seg[0].C = 1, 24, 24
    assert WC.wgrad_shape(d) == 1
    for what, d in WC.rejected_descriptors():
        assert WC.wgrad_splits(d) == -1 and WC.wgrad_shape(d) == -1, what


# ---------------------------------------------------------------------------------------------
# the f64 references, the planted inputs and the argument contracts of tests/test_gpu_boundary_abi.py
# ---------------------------------------------------------------------------------------------
def test_boundary_layout_and_im2col_references_equal_pytorch():
    """nchw <-> nhwc against permute (time-major order through a transposed view) and the first-layer gather against F.unfold,
    in f64, exactly; pad channels / pad taps exactly zero.  The over-the-cap shapes are left to the GPU test."""
    import torch.nn.functional as F
    import boundary_cases as BC
    for case in BC.LAYOUT_CASES:
        if case in BC.LAYOUT_OVER_CAP:
            continue
        n_img, Cc, Cp, H, W, inner = case
        x = BC.layout_input(case, torch.bfloat16).double()
        x = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
        ordered = x.view(inner, n_img // inner, Cc, H, W).transpose(0, 1).reshape(n_img, Cc, H, W)
        got = BC.nchw_to_nhwc_ref(x, Cp, inner)
        assert torch.equal(got, F.pad(ordered.permute(0, 2, 3, 1), (0, Cp - Cc))), case
        assert torch.equal(BC.nhwc_to_nchw_ref(got, Cc), ordered), case
        assert BC.layout_strides(case) == (inner, Cc * H * W, (n_img // inner) * Cc * H * W)
    for n_img, Cc, Cp, H, W in BC.LAYOUT_F32_CASES[:3]:
        x = torch.randn(n_img, Cc, H, W, dtype=torch.float64)
        got = BC.nchw_to_nhwc_ref(x, Cp)
        assert torch.equal(got, F.pad(x.permute(0, 2, 3, 1), (0, Cp - Cc))) and torch.equal(BC.nhwc_to_nchw_ref(got, Cc), x)
    for case in BC.IM2COL_CASES:
        if case in BC.IM2COL_OVER_CAP:
            continue
        n_img, Cc, Kp, H, W, inner = case
        BC.manual_seed(7, *case)
        x = torch.randn(n_img, Cc, H, W, dtype=torch.float64)
        ordered = x.view(inner, n_img // inner, Cc, H, W).transpose(0, 1).reshape(n_img, Cc, H, W)
        cols = F.unfold(ordered, 3, padding=1).view(n_img, Cc, 9, H, W).permute(0, 3, 4, 2, 1).reshape(n_img, H, W, 9 * Cc)
        assert torch.equal(BC.im2col_ref(x, Kp, inner), F.pad(cols, (0, Kp - 9 * Cc))), case
    # C = 3, 5, 7: a tap boundary inside an 8-element chunk; one-row and one-column images
    assert {c[1] for c in BC.IM2COL_CASES} >= {1, 2, 3, 5, 7} and any(c[3] == 1 for c in BC.IM2COL_CASES) and any(c[4] == 1 for c in BC.IM2COL_CASES)


def test_boundary_maxpool_reference_equals_pytorch_autograd():
    """Both directions against F.max_pool2d and its autograd in f64 (ATen routes a tie to the first element in scan order), with and
    without the fused second gradient, on inputs that hold every non-empty subset of the four window positions as the set of
    maximal elements, in the windows and channels the pattern table names."""
    import torch.nn.functional as F
    import boundary_cases as BC
    nchw = lambda t: t.permute(0, 3, 1, 2)
    for case in BC.MAXPOOL_CASES:
        if case in BC.MAXPOOL_OVER_CAP:
            continue
        for dtype in (torch.bfloat16, torch.float16):
            n_img, H, W, Cp = case
            a = BC.maxpool_input(case, dtype).double()
            # the planted sets are the sets of maximal elements
            w = BC.windows(a)
            pat = BC.maxpool_pattern(case)
            at_max = sum((w[k] == w.max(0).values).long() << k for k in range(4))
            assert bool((at_max[pat != 0] == pat[pat != 0]).all()), case
            want_patterns = set(range(1, 16)) if pat.numel() >= 16 else set(range(1, pat.numel()))
            assert set(at_max.flatten().tolist()) >= want_patterns, case
            p, best = BC.maxpool_ref(a)
            dp = torch.randn(p.shape, dtype=torch.float64)
            leaf = nchw(a).clone().requires_grad_(True)
            pooled = F.max_pool2d(leaf, 2)
            (pooled * nchw(dp)).sum().backward()
            assert torch.equal(nchw(p), pooled.detach()), case
            da, written = BC.maxpool_bwd_ref(a, dp)
            assert torch.equal(nchw(da), leaf.grad), case
            assert int(written.sum()) == n_img * (H // 2) * (W // 2) * 4 and bool((da[~written] == 0).all())
            if case in BC.MAXPOOL_ADD_CASES:
                add = torch.randn(a.shape, dtype=torch.float64)
                da2, written2 = BC.maxpool_bwd_ref(a, dp, add)
                assert bool(written2.all()) and torch.equal(da2, add + da)
    assert all(c[1] % 2 == 0 and c[2] % 2 == 0 for c in BC.MAXPOOL_ADD_CASES) and len(BC.MAXPOOL_ADD_CASES) == 3
    assert {(c[1] % 2, c[2] % 2) for c in BC.MAXPOOL_CASES} == {(0, 0), (1, 0), (0, 1), (1, 1)}


def test_boundary_outconv_reference_equals_pytorch_autograd():
    """y, da, dw and db against F.conv2d with a 1x1 kernel and its autograd in f64; the magnitudes bound the values; the lane table
    and the chain lengths of the forward bound."""
    import torch.nn.functional as F
    import boundary_cases as BC
    small = lambda c: c[0] * c[1] <= 4096
    for case in [c for c in BC.OUTCONV_FWD_CASES + BC.OUTCONV_DA_CASES if small(c)] + [c + (None,) for c in BC.OUTCONV_DW_CASES if small(c)]:
        n_img, HW, Cc, Cp, Co = case[:5]
        a, w, b, dy = BC.outconv_operands(case, torch.bfloat16)
        assert bool((a[:, Cc:] == 0).all())
        leaf_a = a.double().view(n_img, HW, 1, Cp).permute(0, 3, 1, 2)[:, :Cc].clone().requires_grad_(True)
        leaf_w, leaf_b = w.double()[:, :, None, None].clone().requires_grad_(True), b.double().clone().requires_grad_(True)
        y = F.conv2d(leaf_a, leaf_w, leaf_b)
        (y * dy.double().view(n_img, Co, HW, 1)).sum().backward()
        ref_y, mag_y = BC.outconv_fwd_ref(a, w, b, n_img, HW)
        torch.testing.assert_close(ref_y, y.detach().view(n_img, Co, HW), rtol=1e-12, atol=1e-12)
        ref_nb, mag_nb = BC.outconv_fwd_ref(a, w, None, n_img, HW)
        torch.testing.assert_close(ref_nb + b.double()[None, :, None], ref_y, rtol=1e-12, atol=1e-12)
        da, da_mag, dw, dw_terms, db, db_terms = BC.outconv_bwd_ref(a, w, dy, Cp)
        torch.testing.assert_close(da[:, :Cc], leaf_a.grad.permute(0, 2, 3, 1).reshape(n_img * HW, Cc), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dw, leaf_w.grad[:, :, 0, 0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(db, leaf_b.grad, rtol=1e-12, atol=1e-12)
        assert bool((da[:, Cc:] == 0).all()) and bool((da_mag[:, Cc:] == 0).all())
        for v, m in ((ref_y, mag_y), (da, da_mag), (dw, dw_terms), (db, db_terms)):
            assert bool((m >= v.abs() * (1 - 1e-12)).all())
    assert [BC.outconv_lanes(Cp) for Cp in (8, 16, 24, 32, 64, 128, 200, 256, 512)] == [0, 2, 0, 4, 8, 16, 0, 32, 0]
    assert BC.outconv_fwd_chain(12, 16) == 10 and BC.outconv_fwd_chain(250, 256) == 14 and BC.outconv_fwd_chain(200, 200) == 201
    assert [BC.outconv_dw_blocks(c[0] * c[1]) for c in BC.OUTCONV_DW_CASES] == [1, 3, 1, 1, 1024]
    assert sum(c[5] is False for c in BC.OUTCONV_FWD_CASES) == 2 and \
        {BC.outconv_lanes(c[3]) > 0 for c in BC.OUTCONV_FWD_CASES if not c[5]} == {True, False}


def test_boundary_attention_reference_equals_the_oracle_autograd():
    """out, dx and dw against oracle.unet_oracle.spatial_attention and its autograd in f64 (torch.max(dim=1) routes the gradient to
    the first maximal channel), and the planted ties are where the table says: the first of the tied channels is the arg-max."""
    import boundary_cases as BC
    from oracle import unet_oracle as O
    kinds = set()
    for case in BC.ATTN_CASES:
        if case[0] * case[1] * case[2] > 1024:
            continue
        n_img, H, W, Cc, Cp, k = case
        x, planted = BC.attn_input(case, torch.bfloat16)
        assert bool((x[..., Cc:] == 0).all())
        w = BC.attn_weight(case).double()
        dout = torch.randn(n_img, H, W, Cp, dtype=torch.float64)
        fwd = BC.attn_fwd_ref(x, w, Cc)
        bwd = BC.attn_bwd_ref(x, dout, w, Cc, fwd)
        arg, mx = fwd["arg"].view(-1), fwd["max"].view(-1)
        for pix, (kind, first) in planted.items():
            kinds.add(kind)
            if first is None:
                assert mx[pix] < 0 and bool((x.view(-1, Cp)[pix, Cc:] == 0).all()) and Cp > Cc, (case, kind)
            else:
                assert int(arg[pix]) == first and int((x.view(-1, Cp)[pix, :Cc] == mx[pix]).sum()) == 2, (case, kind)
        leaf = x.double().permute(0, 3, 1, 2)[:, :Cc].clone().requires_grad_(True)
        leaf_w = w[None].clone().requires_grad_(True)
        out = O.spatial_attention(leaf, {"sa.conv.weight": leaf_w}, "sa")
        (out * dout.permute(0, 3, 1, 2)[:, :Cc]).sum().backward()
        torch.testing.assert_close(fwd["out"][..., :Cc], out.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(bwd["dx"][..., :Cc], leaf.grad.permute(0, 2, 3, 1), rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(bwd["dw"], leaf_w.grad[0], rtol=1e-11, atol=1e-11)
        assert bool((bwd["dx"][..., Cc:] == 0).all()) and bool((fwd["out"][..., Cc:] == 0).all())
    assert kinds == {"one chunk", "two lanes", "two rounds", "first and last channel", "negative beside zero pads"}
    assert {c[5] for c in BC.ATTN_CASES} >= {1, 3, 7, 15}


def test_boundary_loss_gradient_reference_equals_the_oracle_autograd():
    """The closed form of the loss gradient against f64 autograd of oracle.unet_oracle.compute_loss, masked and unmasked (the
    unmasked gradient term of a one-row or one-column plane is an empty mean and is left out); the inputs sit on the 1/64 grid, so
    every difference is exact in f32, and sign(0) occurs in the L1 term and in both kinds of gradient term."""
    import boundary_cases as BC
    from oracle import unet_oracle as O
    for case in BC.LOSS_BWD_CASES:
        if case in BC.LOSS_BWD_OVER_CAP:
            continue
        planes, H, W = case
        for masked in (False, True):
            yp, y, mask = BC.loss_input(case, masked)
            for t in (yp, y):
                assert bool(((t * 64).round() == t * 64).all()) and float(t.abs().max()) <= 4.0
            d = yp - y
            assert torch.equal(d.double(), yp.double() - y.double())
            if planes * H * W >= 64:
                assert bool((d == 0).any())
                if H > 1 and W > 1:
                    assert bool((d[:, :-1, 1:] == d[:, :-1, :-1]).any()) and bool((d[:, 1:, :-1] == d[:, :-1, :-1]).any())
            if masked:
                assert set(mask.flatten().tolist()) <= set(BC.MASK_VALUES)
            elif H == 1 or W == 1:
                continue
            leaf = yp.double().view(planes, 1, 1, H, W).clone().requires_grad_(True)
            y5 = y.double().view(planes, 1, 1, H, W)
            m5 = mask.double().view(planes, 1, 1, H, W) if masked else None
            O.compute_loss(leaf, y5, m5, use_mask=masked).backward()
            wgt = 1.0 + 4.0 * y5.abs() ** 3
            if masked:
                c1 = 1.0 / float((m5 * wgt).sum() + 1e-8)
                c2 = 0.005 / float(m5[..., :H - 1, :W - 1].sum() + 1e-8)
            else:
                c1, c2 = 1.0 / (planes * H * W), 0.005 / (planes * (H - 1) * (W - 1))
            ref, mag = BC.loss_bwd_ref(yp, y, mask, c1, c2)
            torch.testing.assert_close(ref, leaf.grad.view(planes, H, W), rtol=1e-12, atol=1e-15, msg=lambda s: f"{case} {masked}: {s}")
            assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_boundary_kernel_contracts_are_checked_before_launch():
    """UCLSTM_E_BADARG from the shape or the alignment alone: every pointer is a non-null, 16-byte aligned address that is never
    dereferenced because nothing is launched; each call differs from an accepted shape in the one thing named."""
    P, ODD = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 8)
    big = 1 << 16
    for K in (L.lib, L.lib16):
        # layout converters: (n_img, C, Cp, H, W)
        assert K.uclstm_nchw_to_nhwc(P, P, 6, 5, 12, 4, 4, 1, 80, 480, None) == -1            # Cp % 8
        assert K.uclstm_nchw_to_nhwc(P, P, 6, 9, 8, 4, 4, 1, 144, 864, None) == -1            # Cp < C
        assert K.uclstm_nchw_to_nhwc(P, P, 6, 5, 8, 4, 4, 4, 80, 480, None) == -1             # inner does not divide n_img
        assert K.uclstm_nchw_to_nhwc(P, P, 6, 5, 8, 4, 4, 0, 80, 480, None) == -1
        assert K.uclstm_nchw_to_nhwc(P, ODD, 6, 5, 8, 4, 4, 1, 80, 480, None) == -1           # misaligned activation
        assert K.uclstm_nchw_to_nhwc(None, P, 6, 5, 8, 4, 4, 1, 80, 480, None) == -1
        assert K.uclstm_nchw_to_nhwc(P, P, 8, 8, 8, big, big // 2, 1, 0, 0, None) == -1       # 2^31 items
        assert K.uclstm_nchw_grad_to_nhwc(P, P, 6, 5, 12, 4, 4, None) == -1
        assert K.uclstm_nchw_grad_to_nhwc(P, ODD, 6, 5, 8, 4, 4, None) == -1
        assert K.uclstm_nhwc_to_nchw(P, P, 6, 5, 12, 4, 4, None) == -1
        assert K.uclstm_nhwc_to_nchw(ODD, P, 6, 5, 8, 4, 4, None) == -1
        assert K.uclstm_nhwc_to_nchw(P, P, 8, 8, 8, big, big // 2, None) == -1
        # im2col: (n_img, C, Kp, H, W, inner)
        assert K.uclstm_im2col3x3_first(P, P, 6, 2, 16, 4, 4, 1, 32, 192, None) == -1         # Kp < 9*C
        assert K.uclstm_im2col3x3_first(P, P, 6, 2, 20, 4, 4, 1, 32, 192, None) == -1         # Kp % 8
        assert K.uclstm_im2col3x3_first(P, P, 6, 2, 24, 4, 4, 4, 32, 192, None) == -1         # inner
        assert K.uclstm_im2col3x3_first(P, ODD, 6, 2, 24, 4, 4, 1, 32, 192, None) == -1
        assert K.uclstm_im2col3x3_first(P, P, 8, 1, 16, big, big // 4, 1, 0, 0, None) == -1   # 2^31 items
        # MaxPool: (n_img, H, W, Cp)
        assert K.uclstm_maxpool2_fwd(P, P, 2, 4, 4, 12, None) == -1
        assert K.uclstm_maxpool2_fwd(ODD, P, 2, 4, 4, 8, None) == -1
        assert K.uclstm_maxpool2_fwd(P, P, 2, 1, 4, 8, None) == -1                            # no window
        assert K.uclstm_maxpool2_fwd(P, P, 8, 2 * big, big, 8, None) == -1                    # 2^31 chunks
        assert K.uclstm_maxpool2_bwd(P, P, None, P, 2, 4, 4, 12, None) == -1
        assert K.uclstm_maxpool2_bwd(P, P, P, P, 2, 5, 4, 8, None) == -1                      # add with odd H
        assert K.uclstm_maxpool2_bwd(P, P, P, P, 2, 4, 7, 8, None) == -1                      # add with odd W
        assert K.uclstm_maxpool2_bwd(P, P, ODD, P, 2, 4, 4, 8, None) == -1
        assert K.uclstm_maxpool2_bwd(P, P, None, ODD, 2, 4, 4, 8, None) == -1
        assert K.uclstm_maxpool2_bwd(P, P, None, P, 8, 2 * big, big, 8, None) == -1
        # OutConv: (n_img, HW, Cp, C, Co)
        assert K.uclstm_outconv_fwd(P, P, P, P, 2, 16, 12, 12, 1, None) == -1                 # Cp % 8
        assert K.uclstm_outconv_fwd(P, P, P, P, 2, 16, 8, 9, 1, None) == -1                   # C > Cp
        assert K.uclstm_outconv_fwd(ODD, P, P, P, 2, 16, 8, 5, 1, None) == -1
        assert K.uclstm_outconv_fwd(P, P, P, P, 2, 16, 8, 5, 0, None) == -1
        assert K.uclstm_outconv_fwd(P, P, P, P, big, big // 2, 8, 5, 1, None) == -1           # 2^31 pixels
        assert K.uclstm_outconv_bwd(P, P, P, P, P, P, 2, 16, 2056, 2056, 1, None) == -1       # Cp / 8 > 256
        assert K.uclstm_outconv_bwd(P, P, P, P, P, P, 2, 16, 12, 12, 1, None) == -1
        assert K.uclstm_outconv_bwd(ODD, P, P, P, P, P, 2, 16, 8, 5, 1, None) == -1
        assert K.uclstm_outconv_bwd(P, P, P, ODD, P, P, 2, 16, 8, 5, 1, None) == -1
        assert K.uclstm_outconv_bwd(P, P, P, P, P, P, big, big // 2, 8, 5, 1, None) == -1     # 2^31 chunks
        # attention: (n_img, H, W, Cp, C, k)
        for k in (0, 2, 4, 16, 17, -1):
            assert K.uclstm_attention_fwd(P, P, P, P, P, P, 2, 4, 4, 8, 5, k, None) == -1, k
            assert K.uclstm_attention_bwd(P, P, P, P, P, P, P, P, 0, P, 2, 4, 4, 8, 5, k, None) == -1, k
        assert K.uclstm_attention_fwd(P, P, P, P, P, P, 2, 4, 4, 12, 5, 3, None) == -1
        assert K.uclstm_attention_fwd(P, P, P, P, P, P, 2, 4, 4, 8, 9, 3, None) == -1
        assert K.uclstm_attention_fwd(ODD, P, P, P, P, P, 2, 4, 4, 8, 5, 3, None) == -1
        assert K.uclstm_attention_fwd(P, P, ODD, P, P, P, 2, 4, 4, 8, 5, 3, None) == -1
        assert K.uclstm_attention_fwd(P, P, P, P, C.c_void_p((1 << 20) + 4), P, 2, 4, 4, 8, 5, 3, None) == -1     # desc: float2 loads
        assert K.uclstm_attention_fwd(P, P, P, P, P, P, 8, big, big // 4, 8, 5, 3, None) == -1                    # 2^31 chunks
        assert K.uclstm_attention_bwd(P, P, P, P, P, P, P, P, 0, P, 2, 4, 4, 12, 5, 3, None) == -1
        assert K.uclstm_attention_bwd(P, ODD, P, P, P, P, P, P, 0, P, 2, 4, 4, 8, 5, 3, None) == -1
        assert K.uclstm_attention_bwd(P, P, P, P, P, P, ODD, P, 0, P, 2, 4, 4, 8, 5, 3, None) == -1
        assert K.uclstm_attention_bwd(P, P, P, P, P, P, P, P, 0, None, 2, 4, 4, 8, 5, 3, None) == -1              # scratch required
        assert K.uclstm_attention_bwd(P, P, P, P, P, P, P, P, 0, P, 8, big, big // 4, 8, 5, 3, None) == -1
    # the f32 pair and the loss gradient exist once
    assert L.lib.uclstm_nchw_to_nhwc_f32(P, P, 2, 9, 8, 4, 4, None) == -1
    assert L.lib.uclstm_nhwc_to_nchw_f32(P, P, 2, 9, 8, 4, 4, None) == -1
    assert L.lib.uclstm_nchw_to_nhwc_f32(P, None, 2, 5, 8, 4, 4, None) == -1
    assert L.lib.uclstm_nchw_to_nhwc_f32(P, P, 8, 5, 8, big, big // 2, None) == -1
    assert L.lib.uclstm_nhwc_to_nchw_f32(P, P, 8, 8, 8, big, big // 2, None) == -1
    assert L.lib.uclstm_loss_bwd(P, P, None, None, P, 3, 8, 8, None) == -1                    # coefs required
    assert L.lib.uclstm_loss_bwd(P, P, None, P, P, 3, 0, 8, None) == -1
    assert L.lib.uclstm_loss_bwd(P, P, None, P, P, 2, big, big // 4, None) == -1              # 2^31 elements
