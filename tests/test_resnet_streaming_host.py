"""What frame-by-frame inference of PretrainedTemporalUNet promises without a device: the refusals of PretrainedStreamingPredictor and
step_nhwc that come before any device work, StreamingPredictor's unchanged constructor contract after the two predictors were
given a common base, the new entry points in header, binding and library, and the launch plans the GPU suites rely on (the
validation-only planner runs on the host)."""
import ctypes as C
import inspect
import re

import pytest
import torch

import igemm_cases as IC
import test_gpu_igemm_tap_group as TG
import test_gpu_lstm_tick as TK
import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import streaming as S


class FakeDevice(torch.Tensor):          # the shape checks come before any device work: a CPU tensor that says it is on the device
    is_cuda = True


def test_new_entry_points_in_header_binding_and_library():
    hdr = open(L.HEADER_PATH).read()
    syms = set(L.header_symbols())
    raw = C.CDLL(L.LIB_PATH)
    for name in ("uclstm_igemm_fwd_group_tap", "uclstm_igemm_fwd_group_tap_blocks"):
        assert name in syms and name in L._PROTOS and hasattr(raw, name), name
    listed = re.search(r"#define UCLSTM_TAP_GROUP_F16_TWINS\(TWIN\)(.*?)\nUCLSTM_TAP_GROUP_F16_TWINS\(UCLSTM_F16_TWIN\)", hdr, re.S)
    assert listed and re.findall(r"TWIN\((uclstm_[a-z0-9_]+)\)", listed.group(1)) == L.TAP_GROUP_F16_TWINS == ["uclstm_igemm_fwd_group_tap"]
    assert hasattr(raw, "uclstm_igemm_fwd_group_tap_f16") and not hasattr(raw, "uclstm_igemm_fwd_group_tap_blocks_f16")
    assert L.kernels(torch.float16).uclstm_igemm_fwd_group_tap is not L.lib.uclstm_igemm_fwd_group_tap
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16            # additive change
    assert "PretrainedStreamingPredictor" in U.__all__ and U.PretrainedStreamingPredictor is S.PretrainedStreamingPredictor


def test_tap_group_planner_on_the_cases_of_the_gpu_suite():
    """uclstm_igemm_fwd_group_tap_blocks needs no device: every group of the GPU suite is planned as the sum of its members' grids
    rounded up to 8, every refusal is UCLSTM_E_BADARG, and the patch group entry refuses per-tap members as before."""
    for c in TG.CASES.values():
        assert int(L.lib.uclstm_igemm_fwd_shape(C.byref(IC.dummy_desc(c)))) == c.shape, c.name
    for names in TG.GROUPS.values():
        arr = (L.IgemmDesc * len(names))(*[IC.dummy_desc(TG.CASES[n]) for n in names])
        assert int(L.lib.uclstm_igemm_fwd_group_tap_blocks(arr, len(names))) == TG.blocks_expected([TG.CASES[n] for n in names])
        assert int(L.lib.uclstm_igemm_fwd_group_blocks(arr, len(names))) == TG.BADARG
    for what, (names, n, slab) in TG.REFUSALS.items():
        descs = [IC.dummy_desc(TG.CASES[x]) for x in names]
        for d in descs:
            if not slab:
                d.acc_slab = 0
        arr = (L.IgemmDesc * len(descs))(*descs)
        assert int(L.lib.uclstm_igemm_fwd_group_tap_blocks(arr, n)) == TG.BADARG, what
    assert int(L.lib.uclstm_igemm_fwd_group_tap_blocks(None, 1)) == TG.BADARG
    TG.test_members_are_ordered_by_k_steps_per_block()
    # the patch entry keeps taking its own cases
    arr = (L.IgemmDesc * len(IC.GROUP_B))(*[IC.dummy_desc(c) for c in IC.GROUP_B])
    assert int(L.lib.uclstm_igemm_fwd_group_blocks(arr, len(IC.GROUP_B))) == IC.group_blocks_expected(IC.GROUP_B)
    assert int(L.lib.uclstm_igemm_fwd_group_tap_blocks(arr, len(IC.GROUP_B))) == TG.BADARG


def test_tick_partition_of_the_model_shapes():
    """The five recurrences at 64 x 64, B = 1: two patch-shape steps share one launch, three per-tap steps share the other."""
    log, ks, kinds = TK.expected(TK.MODEL)
    assert kinds == ["patch", "patch", "tap", "tap", "tap"]
    assert log[:2] == [("tick", "patch", 2), ("tick", "tap", 3)] and all(e[1] == "pointwise" for e in log[2:])
    assert sum(e[2] for e in log[2:]) == sum(k > 1 for k in ks)


def test_streaming_predictor_constructor_contract_is_unchanged():
    sig = inspect.signature(S.StreamingPredictor.__init__)
    assert list(sig.parameters) == ["self", "model", "use_graph", "warmup"]
    assert sig.parameters["use_graph"].default is True and sig.parameters["warmup"].default == 2
    with pytest.raises(TypeError, match=r"StreamingPredictor drives a TemporalUNetDualView, got PretrainedTemporalUNet "
                                        r"\(PretrainedTemporalUNet has no frame-by-frame step\)"):
        S.StreamingPredictor(U.PretrainedTemporalUNet())
    with pytest.raises(TypeError, match="TemporalUNetDualView"):
        S.StreamingPredictor(torch.nn.Conv2d(1, 1, 1))
    m = U.TemporalUNetDualView(1, 1, base_ch=8, lstm_layers=2, use_skip_lstm=True).train()
    p = S.StreamingPredictor(m, use_graph=False, warmup=5)
    assert p.model is m and not m.training and p.use_graph is False and p.warmup == 5
    assert p.state is None and p._graphs == [None, None] and p._parity == 0 and p._shape is None
    assert p._state_spec(torch.zeros(3, 2, 32, 64)) == {"temporal": (128, 2, 4, 2), "skip3": (64, 4, 8, 1), "skip2": (32, 8, 16, 1)}
    assert S.StreamingPredictor(U.TemporalUNetDualView(1, 1, base_ch=8))._state_spec(torch.zeros(1, 2, 16, 16)) == {"temporal": (128, 1, 1, 1)}
    for name in ("step", "rollout", "reset", "new_sequence", "state"):
        assert hasattr(S.StreamingPredictor, name) and hasattr(S.PretrainedStreamingPredictor, name)
    assert not issubclass(S.StreamingPredictor, S.PretrainedStreamingPredictor)
    assert not issubclass(S.PretrainedStreamingPredictor, S.StreamingPredictor)


def test_pretrained_predictor_refusals_before_any_device_work():
    with pytest.raises(TypeError, match="PretrainedTemporalUNet"):
        S.PretrainedStreamingPredictor(U.TemporalUNetDualView(1, 1, base_ch=8))
    with pytest.raises(TypeError, match="PretrainedTemporalUNet"):
        S.PretrainedStreamingPredictor(torch.nn.Conv2d(1, 1, 1))
    m = U.PretrainedTemporalUNet(lstm_layers=2).train()
    p = S.PretrainedStreamingPredictor(m)
    assert p.model is m and not m.training and p.use_graph is True and p.warmup == 2 and p.state is None
    with pytest.raises(U.UclstmError, match="device tensor"):
        p.step(torch.zeros(1, 2, 64, 64))
    fake = lambda *s: torch.zeros(*s).as_subclass(FakeDevice)
    for bad in (fake(1, 2, 48, 64), fake(1, 2, 64, 80), fake(1, 3, 64, 64), fake(1, 1, 2, 64, 64), fake(2, 64, 64)):
        with pytest.raises(U.UclstmError, match="multiples of 32"):
            p.step(bad)
    m.train()
    with pytest.raises(U.UclstmError, match="training mode"):
        p.step(fake(1, 2, 64, 64))
    m.eval()
    assert p.state is None and p._shape is None          # a refused frame starts nothing
    assert p._state_spec(torch.zeros(2, 2, 64, 96)) == {"lstm": (512, 2, 3, 2), "skip1": (64, 32, 48, 2), "skip2": (64, 16, 24, 2),
                                                        "skip3": (128, 8, 12, 2), "skip4": (256, 4, 6, 2)}


def test_step_nhwc_refusals_before_any_device_work():
    m = U.PretrainedTemporalUNet().eval()
    fake = lambda *s: torch.zeros(*s).as_subclass(FakeDevice)
    with torch.no_grad():
        with pytest.raises(U.UclstmError, match="device tensor"):
            m.step_nhwc(torch.zeros(1, 2, 64, 64))
        with pytest.raises(U.UclstmError, match=r"\[B, 2, H, W\]"):
            m.step_nhwc(fake(1, 2, 2, 64, 64))
        with pytest.raises(U.UclstmError, match="multiples of 32"):
            m.step_nhwc(fake(1, 2, 48, 64))
    with torch.enable_grad(), pytest.raises(U.UclstmError, match="inference only"):
        m.step_nhwc(fake(1, 2, 64, 64))
    m.encoder.layer3[1].bn2.train()
    assert not m.training
    with torch.no_grad(), pytest.raises(U.UclstmError, match="training mode"):
        m.step_nhwc(fake(1, 2, 64, 64))
    m.eval()
    m.decoder.blocks[0].conv1[1].track_running_stats = False          # batch statistics although in evaluation mode
    with torch.no_grad(), pytest.raises(U.UclstmError, match="training mode"):
        m.step_nhwc(fake(1, 2, 64, 64))
    # forward() is what it was: (y, None) is pinned on the device; here only that its checks did not move
    with pytest.raises(U.UclstmError, match=r"\[B, T, 2, H, W\]"):
        m(fake(1, 2, 64, 64))
