"""CPU-only tests of the ResNet18-encoder model (unet-convlstm_amd/resnet.py, csrc/resnet.hip): the C ABI declares, binds and
exports every new entry point and its fp16 twin, every argument contract is a code before any launch, and the module keeps the
reference's state_dict layout (train/resnet18.py:26-74).  No kernel is launched here."""
import ctypes as C
import re

import pytest
import torch

import resnet_cases as RC

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import build as B
from unet_convlstm_amd import resnet as R

TWINS = ["uclstm_im2col7x7s2_first", "uclstm_maxpool3s2_fwd", "uclstm_bn_add_relu", "uclstm_upsample2_fwd", "uclstm_upsample2_bwd",
         "uclstm_head3x3_fwd", "uclstm_head3x3_bwd"]
ONCE = ["uclstm_head3x3_bwd_ordered_rows", "uclstm_head3x3_bwd_ordered"]
P = 1 << 20          # an aligned dummy pointer


def test_header_binding_and_library_agree_on_the_new_entry_points():
    hdr = open(L.HEADER_PATH).read()
    syms = set(L.header_symbols())
    raw = C.CDLL(L.LIB_PATH)
    listed = re.search(r"#define UCLSTM_RESNET_F16_TWINS\(TWIN\)(.*?)\nUCLSTM_RESNET_F16_TWINS\(UCLSTM_F16_TWIN\)", hdr, re.S)
    assert listed, "the twins of csrc/resnet.hip are declared through UCLSTM_F16_TWIN"
    assert re.findall(r"TWIN\((uclstm_[a-z0-9_]+)\)", listed.group(1)) == TWINS == L.RESNET_F16_TWINS
    for name in TWINS + ONCE:
        assert name in syms and name in L._PROTOS and hasattr(raw, name), name
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr).group(1)
        assert len([a for a in params.split(",") if a.strip()]) == len(L._PROTOS[name]), name
    for name in TWINS:
        assert hasattr(raw, name + "_f16"), name
        assert getattr(L.kernels(torch.float16), name) is not getattr(L.lib, name)
    for name in ONCE:          # one symbol each: the activation type is an argument, not a twin
        assert name not in L.RESNET_F16_TWINS and not hasattr(raw, name + "_f16")
    assert L._RESTYPES["uclstm_head3x3_bwd_ordered_rows"] is C.c_int64
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16 == int(re.search(r"#define UCLSTM_ABI_VERSION (\d+)", hdr).group(1))
    assert "resnet.hip" in B.SOURCES and "resnet.hip" in B.F16_SOURCES
    assert "PretrainedTemporalUNet" in U.__all__ and U.PretrainedTemporalUNet is R.PretrainedTemporalUNet


@pytest.mark.parametrize("lib", [L.lib, L.lib16], ids=["bf16", "fp16"])
def test_every_argument_check_is_a_code_before_any_launch(lib):
    E = -1
    # im2col7x7s2_first(x, out, n_img, C, Kp, H, W, inner, inner_stride, outer_stride, stream)
    f = lib.uclstm_im2col7x7s2_first
    for args in [(None, P, 6, 2, 104, 8, 8, 2, 128, 384), (P, None, 6, 2, 104, 8, 8, 2, 128, 384), (P, P + 8, 6, 2, 104, 8, 8, 2, 128, 384),
                 (P, P, 0, 2, 104, 8, 8, 2, 128, 384), (P, P, 6, 0, 104, 8, 8, 2, 128, 384), (P, P, 6, 2, 96, 8, 8, 2, 128, 384),
                 (P, P, 6, 2, 100, 8, 8, 2, 128, 384), (P, P, 6, 2, 104, 0, 8, 2, 128, 384), (P, P, 6, 2, 104, 8, 0, 2, 128, 384),
                 (P, P, 6, 2, 104, 8, 8, 0, 128, 384), (P, P, 6, 2, 104, 8, 8, 4, 128, 384), (P, P, 1 << 20, 2, 104, 64, 64, 1, 0, 8192)]:
        assert f(*args, None) == E, args
    # maxpool3s2_fwd / upsample2_fwd / upsample2_bwd (p0, p1, n_img, H, W, Cp, stream)
    for f in (lib.uclstm_maxpool3s2_fwd, lib.uclstm_upsample2_fwd, lib.uclstm_upsample2_bwd):
        for args in [(None, P, 3, 5, 6, 8), (P, None, 3, 5, 6, 8), (P + 2, P, 3, 5, 6, 8), (P, P + 2, 3, 5, 6, 8), (P, P, 0, 5, 6, 8),
                     (P, P, 3, 0, 6, 8), (P, P, 3, 5, 0, 8), (P, P, 3, 5, 6, 0), (P, P, 3, 5, 6, 12), (P, P, 1 << 16, 256, 256, 64)]:
            assert f(*args, None) == E, args
    # bn_add_relu(z, scale, shift, r, rscale, rshift, a, pixels, Cp, stream)
    f = lib.uclstm_bn_add_relu
    for args in [(None, P, P, P, P, P, P, 90, 8), (P, P, P, None, P, P, P, 90, 8), (P, P, P, P, P, P, None, 90, 8), (P + 4, P, P, P, P, P, P, 90, 8),
                 (P, P, None, P, P, P, P, 90, 8), (P, None, P, P, P, P, P, 90, 8), (P, P, P, P, P, None, P, 90, 8), (P, P, P, P, None, P, P, 90, 8),
                 (P, P + 4, P, P, P, P, P, 90, 8), (P, P, P, P, P, P + 4, P, 90, 8), (P, P, P, P, P, P, P, 0, 8), (P, P, P, P, P, P, P, 90, 0),
                 (P, P, P, P, P, P, P, 90, 20), (P, P, P, P, P, P, P, 1 << 28, 64)]:
        assert f(*args, None) == E, args
    # head3x3_fwd(a, w, b, y, n_img, H, W, Cp, C, Co, stream)
    f = lib.uclstm_head3x3_fwd
    for args in [(None, P, P, P, 3, 5, 6, 16, 10, 3), (P + 8, P, P, P, 3, 5, 6, 16, 10, 3), (P, None, P, P, 3, 5, 6, 16, 10, 3),
                 (P, P, P, None, 3, 5, 6, 16, 10, 3), (P, P, P, P, 0, 5, 6, 16, 10, 3), (P, P, P, P, 3, 0, 6, 16, 10, 3),
                 (P, P, P, P, 3, 5, 0, 16, 10, 3), (P, P, P, P, 3, 5, 6, 12, 10, 3), (P, P, P, P, 3, 5, 6, 72, 10, 3),
                 (P, P, P, P, 3, 5, 6, 16, 0, 3), (P, P, P, P, 3, 5, 6, 16, 17, 3), (P, P, P, P, 3, 5, 6, 16, 10, 0),
                 (P, P, P, P, 3, 5, 6, 16, 10, 5), (P, P, P, P, 1 << 20, 64, 64, 16, 10, 3)]:
        assert f(*args, None) == E, args
    # head3x3_bwd(a, w, dy, da, dw, db, n_img, H, W, Cp, C, Co, stream)
    f = lib.uclstm_head3x3_bwd
    for args in [(None, P, P, P, P, P, 3, 5, 6, 16, 10, 3), (P, None, P, P, P, P, 3, 5, 6, 16, 10, 3), (P, P, None, P, P, P, 3, 5, 6, 16, 10, 3),
                 (P, P, P, P + 8, P, P, 3, 5, 6, 16, 10, 3), (P, P, P, P, P, P, 0, 5, 6, 16, 10, 3), (P, P, P, P, P, P, 3, 5, 6, 72, 10, 3),
                 (P, P, P, P, P, P, 3, 5, 6, 16, 17, 3), (P, P, P, P, P, P, 3, 5, 6, 16, 10, 5), (P, P, P, P, P, P, 3, 5, 6, 20, 10, 3)]:
        assert f(*args, None) == E, args


def test_ordered_head_backward_contract_and_row_planner():
    f, rows = L.lib.uclstm_head3x3_bwd_ordered, L.lib.uclstm_head3x3_bwd_ordered_rows
    ok = (P, P, P, P, P, P, P, 0, 3, 5, 6, 16, 10, 3)
    for i, v in [(0, None), (1, None), (2, None), (3, P + 8), (4, None), (8, 0), (9, 0), (10, 0), (11, 72), (12, 17), (13, 5)]:
        args = list(ok)
        args[i] = v
        for act in (L.ACT_TYPE_BF16, L.ACT_TYPE_F16):
            assert f(*args, act, None) == -1, (i, v)
    assert f(*ok, 2, None) == -1                                     # unknown activation type
    assert rows(0, 5, 6) == -1 and rows(3, 0, 6) == -1 and rows(3, 5, 0) == -1
    sizes = [1, 2, 2047, 2048, 2049, 4096, 4097, 1 << 16, 1 << 21, (1 << 21) + 1, 1 << 24]
    got = [int(rows(n, 1, 1)) for n in sizes]
    assert got == [min(1024, -(-n // 2048)) for n in sizes] and got == [int(rows(1, n, 1)) for n in sizes] == [int(rows(1, 1, n)) for n in sizes]
    assert got[0] == 1 and got[-1] == 1024


@pytest.mark.parametrize("layers,out_channels", [(1, 1), (2, 3)])
def test_state_dict_layout_matches_the_reference_checkpoints(layers, out_channels):
    m = U.PretrainedTemporalUNet(out_channels=out_channels, lstm_layers=layers)
    sd = m.state_dict()
    table = RC.key_table(out_channels, layers)
    assert set(sd) == set(table), (sorted(set(sd) ^ set(table))[:10])
    assert all(tuple(sd[k].shape) == table[k] for k in table), [k for k in table if tuple(sd[k].shape) != table[k]][:5]
    assert all(v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    # the same module objects under two names: shared storage, each tensor once in parameters()
    assert m.base_model.encoder is m.encoder and m.base_model.decoder is m.decoder and m.base_model.segmentation_head is m.head
    for pa, pb in RC.ALIASES:
        keys = [k for k in sd if k.startswith(pb)]
        assert keys and all(sd[k].data_ptr() == sd[pa + k[len(pb):]].data_ptr() for k in keys)
    params = list(m.parameters())
    assert len({id(p) for p in params}) == len(params) == len({p.data_ptr() for p in params})
    assert len(params) == len([k for k in table if not RC.is_buffer(k) and not k.startswith("base_model.")])
    # BatchNorm hyper-parameters of the reference's containers
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    assert len(bns) == 20 + 10 and all(b.eps == 1e-5 and b.momentum == 0.1 for b in bns)
    # a reference checkpoint loads strictly, values and all
    ref = RC.make_state(7, out_channels, layers)
    m.load_state_dict(ref, strict=True)
    got = m.state_dict()
    assert all(torch.equal(got[k], ref[k]) for k in ref)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in ref.items() if k != "encoder.layer2.0.downsample.0.weight"}, strict=True)


def test_which_parameters_train():
    m = U.PretrainedTemporalUNet(lstm_layers=2)
    named = dict(m.named_parameters())
    frozen = {k for k, p in named.items() if not p.requires_grad}
    assert frozen == {k for k in named if k.startswith(("base_model.encoder.", "encoder.", "lstm_skips.0."))} and frozen
    assert {k for k in named if not RC.is_trainable(k.replace("base_model.encoder.", "encoder.").replace("base_model.decoder.", "decoder.")
                                                    .replace("base_model.segmentation_head.", "head."))} == frozen
    m2 = U.PretrainedTemporalUNet(freeze_encoder=False)
    assert {k for k, p in m2.named_parameters() if not p.requires_grad} == {k for k in dict(m2.named_parameters()) if k.startswith("lstm_skips.0.")}
    # freezing does not change the BatchNorm mode: train() puts the frozen encoder's BatchNorm in training mode, as in the reference
    assert m.train().encoder.bn1.training and not m.eval().encoder.bn1.training


def test_encoder_weights_argument(tmp_path):
    tv = RC.torchvision_resnet18_state(11)
    m = U.PretrainedTemporalUNet(encoder_weights=tv)
    assert torch.equal(m.encoder.conv1.weight, tv["conv1.weight"][:, :2] * 1.5)            # smp's 3 -> 2 channel rule
    assert all(torch.equal(v, tv[k]) for k, v in m.encoder.state_dict().items() if k != "conv1.weight")
    assert not any(p.requires_grad for p in m.encoder.parameters())
    path = tmp_path / "resnet18.pth"
    torch.save(tv, path)
    m2 = U.PretrainedTemporalUNet(encoder_weights=str(path), freeze_encoder=False)
    assert all(torch.equal(a, b) for a, b in zip(m.encoder.state_dict().values(), m2.encoder.state_dict().values()))
    already = {k: v for k, v in m.encoder.state_dict().items()}                              # a 2-channel conv1 is taken as it is
    assert torch.equal(U.PretrainedTemporalUNet(encoder_weights=already).encoder.conv1.weight, m.encoder.conv1.weight)
    with pytest.raises(RuntimeError):
        U.PretrainedTemporalUNet(encoder_weights={k: v for k, v in tv.items() if k != "layer3.1.bn2.weight"})
    # random init: BatchNorm at (1, 0), convolutions kaiming_normal_(fan_out): std = sqrt(2 / (Co * k * k))
    m3 = U.PretrainedTemporalUNet()
    assert all(bool((b.weight == 1).all()) and bool((b.bias == 0).all()) for b in m3.base_model.modules() if isinstance(b, torch.nn.BatchNorm2d))
    w = m3.encoder.layer4[1].conv2.weight
    assert abs(float(w.std()) / (2.0 / (512 * 9)) ** 0.5 - 1) < 0.02 and bool((m3.head[0].bias == 0).all())


def test_input_checks_raise_uclstm_error():
    m = U.PretrainedTemporalUNet()
    with pytest.raises(U.UclstmError, match="device tensor"):
        m(torch.zeros(1, 2, 2, 64, 64))
    with pytest.raises(U.UclstmError):
        U.PretrainedTemporalUNet(out_channels=5)
    with pytest.raises(U.UclstmError):
        U.PretrainedTemporalUNet(out_channels=0)
    with pytest.raises(TypeError, match="TemporalUNetDualView"):
        U.StreamingPredictor(m)

    class FakeDevice(torch.Tensor):          # the shape checks come before any device work: a CPU tensor that says it is on the device
        is_cuda = True

    x48 = torch.zeros(1, 2, 2, 48, 64).as_subclass(FakeDevice)
    with pytest.raises(U.UclstmError, match="multiples of 32"):
        m(x48)
    with pytest.raises(U.UclstmError, match="multiples of 32"):
        m(torch.zeros(1, 2, 2, 64, 80).as_subclass(FakeDevice))
    with pytest.raises(U.UclstmError, match=r"\[B, T, 2, H, W\]"):
        m(torch.zeros(1, 2, 3, 64, 64).as_subclass(FakeDevice))
    unfrozen = U.PretrainedTemporalUNet(freeze_encoder=False)
    with pytest.raises(U.UclstmError, match="unfrozen encoder"):
        unfrozen(torch.zeros(1, 2, 2, 64, 64).as_subclass(FakeDevice))


def test_restatement_agrees_with_the_module_containers_on_the_cpu():
    """The yardstick against torch's own modules: the encoder / decoder / head containers of the model, called as plain nn.Modules
    on the CPU in f64 (what smp's forward does with them), give the restatement's features and output."""
    import torch.nn.functional as F
    m = U.PretrainedTemporalUNet(out_channels=2, lstm_layers=1)
    sd = RC.make_state(3, 2, 1)
    m.load_state_dict(sd)
    m = m.double().eval()
    x = torch.randn(1, 2, 2, 32, 32, dtype=torch.float64)
    ref = RC._Ref(sd, False, torch.float64)
    feats = ref.encoder(x.reshape(2, 2, 32, 32))
    e = m.encoder
    a = e.relu(e.bn1(e.conv1(x.reshape(2, 2, 32, 32))))
    assert torch.allclose(a, feats[0], atol=1e-12)
    a = e.maxpool(a)
    for li, layer in enumerate((e.layer1, e.layer2, e.layer3, e.layer4), start=1):
        for blk in layer:
            idt = a if blk.downsample is None else blk.downsample(a)
            a = F.relu(blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(a))))) + idt)
        assert torch.allclose(a, feats[li], atol=1e-10), li
    y, _ = RC.forward_ref(sd, x, False)
    assert y.shape == (1, 2, 2, 32, 32) and bool(torch.isfinite(y).all()) and float(y.std()) > 1e-3
    # train mode: buffers move, gradients exist for every trainable tensor and for nothing else
    xb, yb, mask = RC.make_batch(5, 1, 2, 32, 32, 2)
    yp, loss, grads, buffers = RC.train_ref(sd, xb, yb, mask)
    assert set(grads) == {k for k in sd if RC.is_trainable(k)} and all(float(g.abs().max()) > 0 for g in grads.values())
    assert set(buffers) == {k for k in sd if RC.is_buffer(k) and not k.startswith("base_model.")}
    assert int(buffers["encoder.bn1.num_batches_tracked"]) == 4


# ---------------------------------------------------------------------------------------------
# the decoder cases of tests/test_gpu_resnet_decoder.py: their references and anchors, checked where no GPU is needed
# ---------------------------------------------------------------------------------------------
DEC_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def check_decoder_case(a, b, dtype, cap):
    """``a``, ``b``: the same case computed twice.  The f64 reference is reproducible to f64 rounding and the anchors to well within
    the margins they are used with (2.5 x and 1.25 x); every input is a value the 16-bit type holds; every tensor has a gradient;
    and no anchor is so large that its bound would let an O(1) error pass -- a condition on the seeds, not a measurement."""
    assert all(v is None or torch.equal(v.to(dtype).float(), v) for v in a["inputs"].values())
    assert set(a["grads"]) == set(b["grads"]) and all(g is not None and bool(torch.isfinite(g).all()) and float(g.norm()) > 0 for g in a["grads"].values())
    assert a["out"].dtype == torch.float64 and RC.rel_l2(b["out"], a["out"]) <= 1e-12
    assert all(RC.rel_l2(b["grads"][k], a["grads"][k]) <= 1e-12 for k in a["grads"])
    anchors = lambda r: {"out": r["anchor_out"], **r["anchor_grads"], **r["anchor_buffers"]}
    aa, ab = anchors(a), anchors(b)
    assert set(aa) == set(ab) and all(abs(aa[k] - ab[k]) <= 1e-3 * aa[k] for k in aa), "the autocast anchor is not reproducible"
    assert all(0 <= v < 1 for v in aa.values())          # 0: a sum of 16-bit values in f32 (the last beta's gradient) can be exact
    worst = max(a["anchor_grads"], key=a["anchor_grads"].get)
    print(f"[anchor] worst per-tensor gradient anchor {a['anchor_grads'][worst]:.4f} ({worst}; cap {cap}), output anchor {a['anchor_out']:.6f}")
    assert a["anchor_grads"][worst] <= cap, f"{worst}: anchor {a['anchor_grads'][worst]:.4f} > {cap}: choose another seed"
    assert a["anchor_out"] <= 2e-2


@pytest.mark.parametrize("mode", RC.DEC_MODES)
@pytest.mark.parametrize("dtype", RC.DEC_DTYPES, ids=lambda d: DEC_NAME[d])
@pytest.mark.parametrize("i", range(5))
def test_decoder_block_references_and_anchors(i, dtype, mode):
    for shape in RC.decoder_block_shapes(i):
        a, b = RC.decoder_block_case(i, shape, dtype, mode), RC.decoder_block_reference(i, shape, dtype, mode)
        assert len(a["grads"]) == 6 + (2 if RC.DEC_SKIP[i] else 1) and len(a["anchor_buffers"]) == (4 if mode == "train" else 0)
        check_decoder_case(a, b, dtype, RC.DEC_ANCHOR_CAP)


@pytest.mark.parametrize("mode", RC.DEC_MODES)
@pytest.mark.parametrize("dtype", RC.DEC_DTYPES, ids=lambda d: DEC_NAME[d])
def test_decoder_chain_reference_and_anchors(dtype, mode):
    a, b = RC.decoder_chain_case(dtype, mode), RC.decoder_chain_reference(dtype, mode)
    assert len(a["grads"]) == 5 + 30 + 2 and len(a["anchor_buffers"]) == (20 if mode == "train" else 0)
    assert tuple(a["out"].shape) == (RC.DEC_CHAIN_N, 1, 64, 64)
    check_decoder_case(a, b, dtype, RC.DEC_CHAIN_ANCHOR_CAP)


def test_decoder_helpers_are_the_forward_of_the_restatement():
    """``_Ref.forward`` goes through ``decoder`` / ``decoder_block``: the chain on given inputs is the blocks one by one and the head."""
    inputs, _ = RC.decoder_chain_inputs(torch.bfloat16)
    ref = RC._Ref(RC.decoder_state(), False, torch.float64)
    x, skips = inputs["x"].double(), [inputs[f"skip{j}"].double() for j in range(4)] + [None]
    a = x
    for i, s in enumerate(skips):
        a = ref.decoder_block(a, s, i)
        assert tuple(a.shape) == (RC.DEC_CHAIN_N, RC.DEC_OUT[i], 4 << i, 4 << i)
    p = ref.p
    assert torch.equal(ref.decoder(x, skips), torch.nn.functional.conv2d(a, p["head.0.weight"], p["head.0.bias"], 1, 1))
