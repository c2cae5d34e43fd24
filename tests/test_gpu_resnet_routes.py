"""PretrainedTemporalUNet route against route: the ways through the ResNet18 encoder that do the same arithmetic (frozen under
no_grad, frozen in grad mode, all stages under autograd, the upper stages only; the whole sequence against frame by frame) must give
the same bits.  The method of tests/test_gpu_conv_stage.py: every comparison runs under ops.deterministic() and is torch.equal, and the
yardstick of each test is one route run twice from the same state, asserted bit-identical first -- only then does "B differs from A"
say something about B.

Only the public surface is used -- the model, ``unfreeze_encoder``, ``model(x)``, ``model.encoder.eval()``, ``step_nhwc``,
``ops.deterministic()``, ``ops.LAUNCH_LOG`` -- with state and batch from tests/resnet_cases.py, so the file says the same about any
arrangement of the code underneath.  Shapes: a square and a non-square map whose layer4 sees 2 x 2 and 2 x 3 pixels (a stride or
parity slip shows there), one and two ConvLSTM layers.
"""
import functools

import pytest
import torch

import resnet_cases as RC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

DEV = "cuda"
CASES = [(2, 2, 64, 64, 1), (1, 3, 64, 96, 2)]
DTYPES = [torch.bfloat16, torch.float16]
PARAMS = [pytest.param(c, d, id=f"B{c[0]}T{c[1]}-{c[2]}x{c[3]}-L{c[4]}-{'bf16' if d == torch.bfloat16 else 'fp16'}") for c in CASES for d in DTYPES]
# route -> (argument of unfreeze_encoder or None for the frozen model, grad mode)
ROUTES = {"A": (None, False), "F": (None, True), "B": ("all", True), "C": (("layer3", "layer4"), True)}
short = lambda k: k.replace("base_model.encoder.", "encoder.").replace("base_model.decoder.", "decoder.").replace("base_model.segmentation_head.", "head.")


@functools.lru_cache(maxsize=None)
def inputs(case):
    B, T, H, W, layers = case
    return RC.make_state(100 + layers, 1, layers), RC.make_batch(200 + H + W, B, T, H, W)


def buffers_of(m):
    sd = {k: v.detach().clone() for k, v in m.state_dict().items() if not k.startswith("base_model.") and RC.is_buffer(k)}
    stats = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    counters = {k: int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")}
    assert len(stats) == 60 and len(counters) == 30
    return stats, counters


def train_run(case, dtype, route):
    """A fresh model in training mode, one forward through ``route`` (and, in grad mode, the loss and its backward pass) under
    ops.deterministic(): y, the BatchNorm buffers, the counters, every gradient by short key, the sorted LAUNCH_LOG of the forward."""
    sd, (x, y, mask) = inputs(case)
    stages, grad = ROUTES[route]
    with ops.deterministic(), ops.compute_dtype(dtype):
        m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=case[4]).to(DEV)
        m.load_state_dict(sd, strict=True)
        if stages is not None:
            m.unfreeze_encoder(stages)
        m.train()
        ops.LAUNCH_LOG = []
        try:
            with torch.set_grad_enabled(grad):
                yp, _ = m(x.to(DEV))
            log = sorted(repr(e) for e in ops.LAUNCH_LOG)
        finally:
            ops.LAUNCH_LOG = None
        if grad:
            U.compute_loss(yp, y.to(DEV), mask.to(DEV), True).backward()
        torch.cuda.synchronize()
    stats, counters = buffers_of(m)
    return dict(y=yp.detach(), stats=stats, counters=counters, log=log, grads={short(k): p.grad for k, p in m.named_parameters()})


cached_run = functools.lru_cache(maxsize=None)(train_run)


def same_forward(a, b, what):
    assert torch.equal(a["y"], b["y"]), f"{what}: y"
    diff = [k for k in a["stats"] if not torch.equal(a["stats"][k], b["stats"][k])]
    assert not diff, f"{what}: BatchNorm buffers differ: {diff[:6]}"
    assert a["counters"] == b["counters"] and set(a["counters"].values()) == {4}, f"{what}: counters"


def above_encoder(grads):
    return {k: g for k, g in grads.items() if not k.startswith(("encoder.", "lstm_skips.0."))}


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_training_mode_three_routes_give_the_same_bits(case, dtype):
    """Frozen under no_grad (A), all stages under autograd (B), layer3 + layer4 under autograd (C): the same forward kernels on the
    same operands, so y, the 60 running statistics and the 30 counters agree in every bit."""
    a = cached_run(case, dtype, "A")
    same_forward(a, train_run(case, dtype, "A"), "A, run to run")
    assert float(a["y"].abs().max()) > 0
    for r in ("B", "C"):
        same_forward(a, cached_run(case, dtype, r), f"{r} against A")


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_frozen_encoder_in_grad_mode_is_route_a_and_its_gradients_are_route_b_s(case, dtype):
    """The ordinary training step (F): its forward is A's, and every gradient above the encoder is that of the all-stages run --
    nothing above the encoder depends on whether the encoder keeps its activations."""
    f = cached_run(case, dtype, "F")
    again = train_run(case, dtype, "F")
    same_forward(f, again, "F, run to run")
    gf, gb = above_encoder(f["grads"]), above_encoder(cached_run(case, dtype, "B")["grads"])
    assert set(gf) == set(gb) and len(gf) > 40 and all(g is not None for g in gf.values())
    assert not [k for k in gf if not torch.equal(gf[k], above_encoder(again["grads"])[k])], "F, run to run: gradients"
    same_forward(cached_run(case, dtype, "A"), f, "F against A")
    diff = [k for k in gf if not torch.equal(gf[k], gb[k])]
    assert not diff, f"gradients above the encoder differ between the frozen and the all-stages run: {diff[:6]}"
    assert all(g is None for k, g in f["grads"].items() if k.startswith("encoder."))
    assert float(max(g.abs().max() for g in gf.values())) > 0


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_forward_launches_are_the_same_multiset(case, dtype):
    """LAUNCH_LOG of the forward pass, compared SORTED, not in sequence: inside a strided block the downsample convolution may be
    launched at a different position on one route than on another, and that is allowed; a launch more, less or of another shape is not."""
    a = cached_run(case, dtype, "A")
    assert a["log"] == train_run(case, dtype, "A")["log"]
    assert len([e for e in a["log"] if e.startswith("('fwd'")]) >= 20 + 10 + 5 * case[1] * case[4]          # encoder, decoder, ConvLSTM steps
    for r in ("F", "B", "C"):
        assert a["log"] == cached_run(case, dtype, r)["log"], f"forward launches of {r} differ from A's"


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_evaluation_fold_whole_sequence_equals_frame_by_frame(case, dtype):
    """Evaluation mode without a backward pass folds BatchNorm into the convolution's epilogue (one rounding), with one it keeps z
    and applies BatchNorm after it (two), so A is not compared with B here.  The fold is pinned to itself: ``model(x)`` under no_grad
    equals the frames fed to ``step_nhwc`` one by one with the state carried, bit for bit, and no buffer moves."""
    sd, (x, _, _) = inputs(case)
    with ops.deterministic(), ops.compute_dtype(dtype), torch.no_grad():
        m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=case[4]).to(DEV)
        m.load_state_dict(sd, strict=True)
        m.eval()
        x = x.to(DEV)
        y, _ = m(x)
        again, _ = m(x)
        frames, state = [], None
        for t in range(x.shape[1]):
            yt, state = m.step_nhwc(x[:, t], state)
            frames.append(yt)
        torch.cuda.synchronize()
    assert torch.equal(y, again), "whole sequence, run to run"
    assert float(y.abs().max()) > 0
    assert torch.equal(y, torch.stack(frames, dim=1)), "step_nhwc frame by frame differs from the whole sequence"
    stats, counters = buffers_of(m)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in stats.items()) and set(counters.values()) == {3}, "a buffer moved in evaluation mode"
