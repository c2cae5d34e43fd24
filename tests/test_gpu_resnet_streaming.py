"""PretrainedStreamingPredictor / PretrainedTemporalUNet.step_nhwc on the GPU: frame-by-frame inference of the shipped model.

Parity is against the functional restatement of tests/resnet_cases.py in f64 on the CPU, run on the WHOLE sequence in evaluation
mode; the bound and its anchor are those tests/test_gpu_resnet_model.py uses for the evaluation forward: per-timestep rel-L2 <= 1.25 x
the drift of the same restatement under torch.autocast("cpu") in the compute type.  Everything else -- graph against eager, chunked
against whole, restart, a fresh predictor after a weight change -- is bit equality.  Measured ratios are printed (run with -s) and
recorded in DESIGN.md section 4.
"""
import functools

import pytest
import torch

import resnet_cases as RC
from conftest import rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

DEV = "cuda"
torch.set_num_threads(16)
CASES = [(2, 4, 64, 64, 2), (1, 3, 64, 96, 1)]
IDS = [f"B{b}T{t}-{h}x{w}-L{l}" for b, t, h, w, l in CASES]
KEYS = ("lstm", "skip1", "skip2", "skip3", "skip4")
CHANNELS = {"lstm": 512, "skip1": 64, "skip2": 64, "skip3": 128, "skip4": 256}
STRIDE = {"lstm": 32, "skip1": 2, "skip2": 4, "skip3": 8, "skip4": 16}


def per_t(got, ref):
    return [rel_l2(got[:, t], ref[:, t]) for t in range(ref.shape[1])]


@functools.lru_cache(maxsize=None)
def reference_f64(case):
    """Computed once per case and shared, never modified: state, batch and the f64 result of the whole sequence."""
    B, T, H, W, layers = case
    sd = RC.make_state(300 + layers, 1, layers)
    x, _, _ = RC.make_batch(400 + H + W, B, T, H, W)
    with torch.no_grad():
        y, _ = RC.forward_ref(sd, x, False)
    return dict(sd=sd, x=x, y=y)


@functools.lru_cache(maxsize=None)
def reference(case, autocast=torch.bfloat16):
    """reference_f64 + the drift of the restatement under autocast in the compute type (the anchor), once per (case, type)."""
    ref = reference_f64(case)
    with torch.no_grad():
        a, _ = RC.forward_ref(ref["sd"], ref["x"], False, torch.float32, autocast)
    return dict(ref, anchor=per_t(a.double(), ref["y"]))


def build(ref, layers):
    m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=layers).to(DEV)
    m.load_state_dict(ref["sd"], strict=True)
    return m.eval()


def check_outputs(what, got, want, anchor):
    e = per_t(got.double().cpu(), want)
    print(f"[parity] {what}: per-timestep rel-L2 {[round(v, 5) for v in e]}; the restatement's own autocast drift {[round(v, 5) for v in anchor]}; "
          f"ratios {[round(v / a, 3) for v, a in zip(e, anchor)]} (bound 1.25)")
    for t, (v, a) in enumerate(zip(e, anchor)):
        assert v <= 1.25 * a, f"{what} t={t}: drift {v:.5f} > 1.25 x the anchor's {a:.5f}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rollout_against_f64_and_state_layout(case):
    B, T, H, W, layers = case
    ref = reference(case)
    m = build(ref, layers)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    p = U.PretrainedStreamingPredictor(m, use_graph=False)
    assert p.state is None
    y = p.rollout(ref["x"].to(DEV))
    assert tuple(y.shape) == tuple(ref["y"].shape) and y.dtype == torch.float32
    check_outputs(f"rollout {case}", y, ref["y"], ref["anchor"])
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items()), "a rollout changed a parameter or a buffer"
    st = p.state
    assert tuple(st) == KEYS
    for k in KEYS:
        assert len(st[k]) == layers
        for h, c in st[k]:
            shape = (B, H // STRIDE[k], W // STRIDE[k], CHANNELS[k])
            assert tuple(h.shape) == tuple(c.shape) == shape and h.dtype == torch.bfloat16 and c.dtype == torch.float32
            assert h.is_contiguous() and c.is_contiguous() and float(h.float().abs().max()) > 0 and float(c.abs().max()) > 0


def test_fp16_rollout_against_f64():
    case = CASES[0]
    ref = reference(case, torch.float16)
    with ops.compute_dtype(torch.float16):
        m = build(ref, case[4])
        p = U.PretrainedStreamingPredictor(m, use_graph=False)
        y = p.rollout(ref["x"].to(DEV))
        assert all(h.dtype == torch.float16 for k in KEYS for h, _ in p.state[k])
    check_outputs(f"fp16 rollout {case}", y, ref["y"], ref["anchor"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_graph_equals_eager_chunks_and_restart(case):
    B, T, H, W, layers = case
    ref = reference_f64(case)
    m = build(ref, layers)
    x = ref["x"].to(DEV)
    xx = torch.cat([x, x.flip(1)], dim=1)                    # 2T frames: both parities are captured whatever T is
    eager = U.PretrainedStreamingPredictor(m, use_graph=False)
    graph = U.PretrainedStreamingPredictor(m, use_graph=True, warmup=2)
    ye = eager.rollout(xx)
    yg = graph.rollout(xx)
    assert all(g is not None for g in graph._graphs), "both state parities are captured after the warm-up"
    for t in range(xx.shape[1]):
        assert torch.equal(ye[:, t], yg[:, t]), f"frame {t}: the captured step differs from the eager step"
    for k in KEYS:
        for (h, c), (h2, c2) in zip(eager.state[k], graph.state[k]):
            assert torch.equal(h, h2) and torch.equal(c, c2)
    # a new sequence on the same buffers and graphs, in two chunks
    graph.new_sequence()
    y2 = torch.cat([graph.rollout(xx[:, :3]), graph.rollout(xx[:, 3:])], dim=1)
    assert torch.equal(y2, yg), "two chunks after new_sequence() differ from one rollout"
    eager.new_sequence()
    assert torch.equal(torch.cat([eager.rollout(xx[:, :1]), eager.rollout(xx[:, 1:])], dim=1), ye)
    # a changed frame shape is refused until reset(), which also restarts the sequence
    with pytest.raises(ValueError, match="frame shape changed"):
        graph.step(torch.zeros(B, 2, H + 32, W, device=DEV))
    graph.reset()
    assert graph.state is None and graph._graphs == [None, None]
    assert torch.equal(graph.rollout(xx), yg)


def test_weight_change_is_followed():
    case = CASES[1]
    B, T, H, W, layers = case
    ref = reference_f64(case)
    m = build(ref, layers)
    x = ref["x"].to(DEV)
    xx = torch.cat([x, x], dim=1)
    p = U.PretrainedStreamingPredictor(m, use_graph=True, warmup=1)
    y0 = p.rollout(xx)
    assert all(g is not None for g in p._graphs)
    with torch.no_grad():
        m.lstm_skips[3].layers[0].conv.weight.mul_(0.5)
        m.lstm.layers[0].conv.bias.add_(0.25)
        m.head[0].bias.add_(0.5)
        m.decoder.blocks[1].conv1[1].running_var.mul_(2.0)
    ops.weights_changed()
    p.new_sequence()
    y1 = p.rollout(xx)
    fresh = U.PretrainedStreamingPredictor(m, use_graph=False)
    assert torch.equal(y1, fresh.rollout(xx)), "after a weight change the predictor does not follow the new weights"
    assert not torch.equal(y1, y0)


def test_refusals():
    ref = reference_f64(CASES[1])
    m = build(ref, 1)
    p = U.PretrainedStreamingPredictor(m, use_graph=False)
    with pytest.raises(U.UclstmError, match="device tensor"):
        p.step(torch.zeros(1, 2, 64, 64))
    with pytest.raises(U.UclstmError, match="multiples of 32"):
        p.step(torch.zeros(1, 2, 48, 64, device=DEV))
    with pytest.raises(U.UclstmError, match="multiples of 32"):
        p.step(torch.zeros(1, 3, 64, 64, device=DEV))
    with pytest.raises(U.UclstmError):
        p.rollout(torch.zeros(1, 2, 64, 64, device=DEV))          # a frame sequence must be [B, T, 2, H, W]
    x = torch.zeros(1, 2, 64, 64, device=DEV)
    with torch.enable_grad(), pytest.raises(U.UclstmError, match="inference only"):
        m.step_nhwc(x)
    bn = m.decoder.blocks[2].conv2[1]
    bn.train()
    assert not m.training
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(U.UclstmError, match="training mode"):
        p.step(x)
    with torch.no_grad(), pytest.raises(U.UclstmError, match="training mode"):
        m.step_nhwc(x)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    bn.eval()
    m.train()
    with pytest.raises(U.UclstmError, match="training mode"):
        p.step(x)
    m.eval()
    assert tuple(p.step(x).shape) == (1, 1, 64, 64)
    with pytest.raises(TypeError, match="PretrainedTemporalUNet"):
        U.PretrainedStreamingPredictor(U.TemporalUNetDualView(1, 1, base_ch=8, lstm_layers=1, use_skip_lstm=True).to(DEV))
    with pytest.raises(TypeError, match="TemporalUNetDualView"):
        U.StreamingPredictor(m)


def test_step_nhwc_without_buffers_equals_the_predictor():
    """step_nhwc with full_state=None (the zero state) and no out_state allocates its own state and chains through what it returns."""
    case = CASES[1]
    ref = reference_f64(case)
    m = build(ref, case[4])
    x = ref["x"].to(DEV)
    want = U.PretrainedStreamingPredictor(m, use_graph=False).rollout(x)
    state = None
    with torch.no_grad():
        for t in range(x.shape[1]):
            y, state = m.step_nhwc(x[:, t], state)
            assert torch.equal(y, want[:, t]), f"frame {t}"
