"""PretrainedTemporalUNet with a trainable encoder (``model.unfreeze_encoder(...)``) on the GPU against the functional restatement
of tests/resnet_cases.py in f64 on the CPU, with ``is_trainable(k, False)``: every encoder tensor gets a gradient.

Tolerances are anchored exactly as in tests/test_gpu_resnet_model.py: the restatement under ``torch.autocast("cpu", bfloat16)``
against its own f64 result, outputs within 1.25 x the anchor per timestep, gradients and BatchNorm buffers through
``conftest.per_tensor_grad_report`` with its defaults.  Measured ratios are printed (run with -s) and recorded in DESIGN.md section 4.
The fp16 case has no anchored tolerance (the fp16 autocast anchor of a training pass has not been shown to run on the CPU): the
kernel-level fp16 checks of tests/test_gpu_resnet_bwd_abi.py carry the numerics, this file checks that fp16 training runs and learns.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_cases as RC
from conftest import per_tensor_grad_report, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops
    from unet_convlstm_amd import resnet as R

DEV = "cuda"
torch.set_num_threads(16)
CASES = [(2, 2, 64, 64, 1), (1, 3, 64, 96, 2)]
IDS = [f"B{b}T{t}-{h}x{w}-L{l}" for b, t, h, w, l in CASES]
ENC_CONVS = 20                                     # convolutions of the ResNet18 encoder: the stem, 16 in the blocks, 3 downsamples
short = lambda k: k.replace("base_model.encoder.", "encoder.").replace("base_model.decoder.", "decoder.").replace("base_model.segmentation_head.", "head.")


class _EncoderEvalRef(RC._Ref):
    """The restatement with evaluation-mode BatchNorm in the encoder only (``model.train(); model.encoder.eval()``)."""

    def bn(self, x, prefix):
        if not prefix.startswith("encoder."):
            return super().bn(x, prefix)
        p = self.p
        return F.batch_norm(x, p[prefix + "running_mean"], p[prefix + "running_var"], p[prefix + "weight"], p[prefix + "bias"], False, 0.1, 1e-5)


def train_ref(sd, x, y, mask, dtype=torch.float64, autocast=None, encoder_eval=False):
    """RC.train_ref with the encoder trainable: (y_pred, loss, {key: grad}, buffers)."""
    names = [k for k in sd if RC.is_trainable(k, False)]
    leaves = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in names}
    ref = (_EncoderEvalRef if encoder_eval else RC._Ref)({**sd, **leaves}, True, dtype)
    with (torch.autocast("cpu", dtype=autocast) if autocast is not None else contextlib.nullcontext()):
        yp = ref.forward(x)
    loss = RC.loss_ref(yp.to(dtype), y.to(dtype), mask.to(dtype))
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return yp.detach(), loss.detach(), dict(zip(names, grads)), ref.buffers


def per_t(got, ref):
    return [rel_l2(got[:, t], ref[:, t]) for t in range(ref.shape[1])]


@functools.lru_cache(maxsize=None)
def reference(case, encoder_eval=False):
    """Computed once per case and shared, never modified: state, batch, the f64 results and the autocast anchor's drift."""
    B, T, H, W, layers = case
    sd = RC.make_state(100 + layers, 1, layers)
    x, y, mask = RC.make_batch(200 + H + W, B, T, H, W)
    y_train, loss, grads, buffers = train_ref(sd, x, y, mask, encoder_eval=encoder_eval)
    a_train, a_loss, a_grads, a_buffers = train_ref(sd, x, y, mask, torch.float32, torch.bfloat16, encoder_eval)
    fbuf = [k for k in buffers if not k.endswith("num_batches_tracked")]
    return dict(sd=sd, x=x, y=y, mask=mask, y_train=y_train, loss=float(loss), grads=grads, buffers=buffers,
                anchor_train=per_t(a_train.double(), y_train), anchor_loss=abs(float(a_loss) - float(loss)) / abs(float(loss)),
                anchor_grads={k: rel_l2(a_grads[k], grads[k]) for k in grads}, anchor_buffers={k: rel_l2(a_buffers[k], buffers[k]) for k in fbuf})


def run_train(case, ref, stages="all", encoder_eval=False):
    """Fresh model, one train-mode forward + backward with LAUNCH_LOG on: (model, y_pred, loss, log of forward, log of backward)."""
    m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=case[4]).to(DEV)
    m.load_state_dict(ref["sd"], strict=True)
    m.unfreeze_encoder(stages)
    m.train()
    if encoder_eval:
        m.encoder.eval()
    for p in m.parameters():
        p.grad = None
    ops.LAUNCH_LOG = []
    try:
        y, _ = m(ref["x"].to(DEV))
        n_fwd = len(ops.LAUNCH_LOG)
        loss = U.compute_loss(y, ref["y"].to(DEV), ref["mask"].to(DEV), True)
        loss.backward()
        torch.cuda.synchronize()
        log = list(ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
    return m, y.detach(), loss.detach(), log[:n_fwd], log[n_fwd:]


@functools.lru_cache(maxsize=None)
def all_stages_run(case):
    """One all-stages step per case, shared by the tests that read it: host copies only."""
    ref = reference(case)
    m, y, loss, log_f, log_b = run_train(case, ref)
    grads = {short(k): (None if p.grad is None else p.grad.cpu()) for k, p in m.named_parameters()}
    return dict(y=y.cpu(), loss=float(loss), log_f=log_f, log_b=log_b, grads=grads, sd={k: v.cpu() for k, v in m.state_dict().items()})


def check_gradients(what, got, ref):
    names = list(ref["grads"])
    assert set(k for k, g in got.items() if g is not None) == set(names), sorted(set(k for k, g in got.items() if g is not None) ^ set(names))[:8]
    bad, rows, med = per_tensor_grad_report(names, got, ref["grads"], [float(ref["grads"][k].norm()) for k in names],
                                            [ref["anchor_grads"][k] for k in names])
    enc = [r for r in rows if r[1].startswith("encoder.")]
    print(f"[parity] {what}: per-tensor gradients: median rel-L2 / anchor {med:.3f} (bound 1.25) over {len(rows)} tensors, {len(enc)} of the encoder; "
          "worst five (rel-L2 / bound): " + "; ".join(f"{k} {rel:.4f}/{bound:.4f}" for _, k, rel, bound, _, z in rows[:5] if not z) +
          "; worst five of the encoder: " + "; ".join(f"{k} {rel:.4f}/{bound:.4f}" for _, k, rel, bound, _, z in enc[:5] if not z))
    assert len(enc) == 60                                  # every encoder tensor is in the report: 20 weights, 20 gammas, 20 betas
    assert not bad, " | ".join(bad[:8])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_all_stages_trainable_gradients(case):
    ref, run = reference(case), all_stages_run(case)
    assert set(ref["grads"]) == {k for k in ref["sd"] if RC.is_trainable(k, False)}
    check_gradients(f"unfrozen {case}", run["grads"], ref)
    assert all(g is None for k, g in run["grads"].items() if k.startswith("lstm_skips.0."))
    # backward launches: a weight-gradient GEMM per convolution, the encoder's 20 included; input-gradient launches: the frozen model's,
    # plus the x half of the five ConvLSTMs that now get an input that requires grad, plus 4 per encoder layer (the stem computes none;
    # a strided block's conv1 and downsample share ONE)
    B, T, H, W, layers = case
    assert not [e for e in run["log_f"] if e[0] == "wgrad"]
    assert len([e for e in run["log_b"] if e[0] == "wgrad"]) == ENC_CONVS + 10 + 5 * layers
    assert len([e for e in run["log_b"] if e[0] == "fwd"]) == 14 + 5 * (layers * (T - 1) + (layers - 1)) + 5 + 16


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_all_stages_trainable_outputs_loss_and_buffers(case):
    ref, run = reference(case), all_stages_run(case)
    e = per_t(run["y"].double(), ref["y_train"])
    print(f"[parity] unfrozen train {case}: per-timestep rel-L2 {[round(v, 5) for v in e]}; anchor {[round(v, 5) for v in ref['anchor_train']]}; "
          f"ratios {[round(v / a, 3) for v, a in zip(e, ref['anchor_train'])]} (bound 1.25)")
    assert all(v <= 1.25 * a for v, a in zip(e, ref["anchor_train"]))
    dl = abs(run["loss"] - ref["loss"]) / abs(ref["loss"])
    print(f"[parity] unfrozen train {case}: loss {run['loss']:.6f} vs f64 {ref['loss']:.6f} (rel {dl:.2e}; anchor {ref['anchor_loss']:.2e})")
    assert dl <= max(1.25 * ref["anchor_loss"], 5e-3)
    sd = run["sd"]
    counters = [k for k in ref["buffers"] if k.endswith("num_batches_tracked")]
    assert len(counters) == 30 and all(int(sd[k]) == int(ref["buffers"][k]) == 4 for k in counters)
    names = list(ref["anchor_buffers"])
    assert len(names) == 60
    bad, rows, med = per_tensor_grad_report(names, sd, ref["buffers"], [float(ref["buffers"][k].double().norm()) for k in names],
                                            [ref["anchor_buffers"][k] for k in names])
    print(f"[parity] unfrozen train {case}: BatchNorm buffers: median rel-L2 / anchor {med:.3f} (bound 1.25)")
    assert not bad, " | ".join(bad[:8])


def test_partial_unfreeze_is_bit_identical_and_launches_nothing_below():
    case = CASES[1]
    B, T, H, W, layers = case
    ref = reference(case)
    with ops.deterministic():
        full, _, _, _, _ = run_train(case, ref)
        part, _, _, log_f, log_b = run_train(case, ref, ("layer3", "layer4"))
    gf = {short(k): p.grad for k, p in full.named_parameters()}
    trainable = 0
    for k, p in part.named_parameters():
        k = short(k)
        if k.startswith("encoder.") and not k.startswith(("encoder.layer3.", "encoder.layer4.")):
            assert p.grad is None and not p.requires_grad, k
        elif k.startswith("encoder."):
            trainable += 1
            assert p.grad is not None and torch.equal(p.grad, gf[k]), f"{k}: differs from the all-stages run"
        elif not k.startswith("lstm_skips.0."):
            # above the encoder nothing depends on which encoder stages train
            assert p.grad is not None and torch.equal(p.grad, gf[k]), f"{k}: differs from the all-stages run"
    assert trainable == 30
    # weight-gradient GEMMs: the 10 convolutions of layer3 and layer4 only; input-gradient launches: none below layer3.0 -- 3 in
    # layer3 (its first conv1 / downsample get no input gradient), 4 in layer4, and the x half of the two ConvLSTMs on f4 and f5
    assert len([e for e in log_b if e[0] == "wgrad"]) == 10 + 10 + 5 * layers
    assert len([e for e in log_b if e[0] == "fwd"]) == 14 + 5 * (layers * (T - 1) + (layers - 1)) + 2 + 7
    assert not [e for e in log_f if e[0] == "wgrad"]


def test_evaluation_statistics_with_backward():
    case = CASES[0]
    ref = reference(case, True)
    m, y, loss, _, _ = run_train(case, ref, "all", encoder_eval=True)
    e = per_t(y.double().cpu(), ref["y_train"])
    print(f"[parity] encoder.eval() {case}: per-timestep rel-L2 {[round(v, 5) for v in e]}; anchor {[round(v, 5) for v in ref['anchor_train']]}")
    assert all(v <= 1.25 * a for v, a in zip(e, ref["anchor_train"]))
    check_gradients(f"encoder.eval() {case}", {short(k): (None if p.grad is None else p.grad.cpu()) for k, p in m.named_parameters()}, ref)
    sd = m.state_dict()
    enc_buffers = [k for k in ref["sd"] if k.startswith("encoder.") and RC.is_buffer(k)]
    assert len(enc_buffers) == 60 and all(torch.equal(sd[k].cpu(), ref["sd"][k]) for k in enc_buffers), "encoder buffers moved"
    assert not [k for k in ref["buffers"] if k.startswith("encoder.")]
    assert all(int(sd[k]) == 4 for k in ref["buffers"] if k.endswith("num_batches_tracked"))          # the decoder's still count


def test_deterministic_mode_is_bit_exact():
    case = CASES[1]
    ref = reference(case)
    runs = []
    with ops.deterministic():
        for _ in range(2):
            m, y, loss, log_f, log_b = run_train(case, ref)
            kinds = {e[1] for e in log_f + log_b if e[0] == "reduce"}
            assert "head3x3_bwd_ordered" in kinds and not kinds & set(R.ATOMIC_KINDS), kinds
            runs.append((loss.cpu(), y.cpu(), {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None}))
    (l0, y0, g0), (l1, y1, g1) = runs
    assert torch.equal(l0, l1) and torch.equal(y0, y1) and set(g0) == set(g1) and len(g0) > 100
    diff = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not diff, f"gradients differ between two runs in deterministic mode: {diff[:6]}"


def two_group_optimizer(m, lr, **kw):
    enc = [p for p in m.encoder.parameters() if p.requires_grad]
    rest = [p for n, p in m.named_parameters() if p.requires_grad and ".encoder." not in n and not n.startswith("encoder.")]
    return U.FusedAdamW([{"params": enc, "lr": lr / 10}, {"params": rest}], lr=lr, weight_decay=1e-2, max_grad_norm=1.0, order=m.parameters(), **kw)


def test_ten_train_steps_with_the_two_group_optimiser():
    case = CASES[1]
    ref = reference(case)
    m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=case[4]).to(DEV)
    m.load_state_dict(ref["sd"], strict=True)
    m.unfreeze_encoder(("layer3", "layer4")).train()
    opt = two_group_optimizer(m, 1e-3)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    x, y, mask = ref["x"].to(DEV), ref["y"].to(DEV), ref["mask"].to(DEV)
    losses = [float(U.train_step(m, opt, x, y, mask, True)[0]) for _ in range(10)]
    print(f"[train] ten steps, layer3 + layer4 unfrozen at lr / 10: losses {[round(v, 5) for v in losses]}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    for k, p in m.named_parameters():
        if p.requires_grad and "encoder." in k and k.endswith("weight"):
            assert not torch.equal(p.detach(), before[k]), f"{k} did not change"
        if not p.requires_grad:
            assert torch.equal(p.detach(), before[k]) and p.grad is None, k
    assert int(m.encoder.bn1.num_batches_tracked) == 3 + 10


def test_fp16_five_steps_with_loss_scaling():
    case = CASES[0]
    ref = reference(case)
    with ops.compute_dtype(torch.float16):
        m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=case[4]).to(DEV)
        m.load_state_dict(ref["sd"], strict=True)
        m.unfreeze_encoder("all").train()
        opt = two_group_optimizer(m, 1e-3, loss_scale=2 ** 14)
        x, y, mask = ref["x"].to(DEV), ref["y"].to(DEV), ref["mask"].to(DEV)
        losses = [float(U.train_step(m, opt, x, y, mask, True)[0]) for _ in range(5)]
    print(f"[train] fp16, five steps, all stages unfrozen: losses {[round(v, 5) for v in losses]}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


# ---------------------------------------------------------------------------------------------
# single stages: where the whole model's own reduced-precision drift is large (per-tensor anchors of 0.4 .. 0.9 above), one block on
# 6 x 8 x 8 inputs is not chaotic -- a wrong wiring (parity order, a missing term, a wrong tensor) is O(1) against anchors of a few per cent
# ---------------------------------------------------------------------------------------------
BLOCKS = [("layer1", 0), ("layer2", 0), ("layer3", 0), ("layer4", 1)]          # identity residual, strided with downsample (one and two chunks)


stage_grads, report = RC.stage_grads, RC.report          # shared with tests/test_gpu_resnet_decoder.py


@pytest.mark.parametrize("block", BLOCKS, ids=lambda b: f"{b[0]}.{b[1]}")
def test_one_basic_block_against_f64(block):
    name, idx = block
    prefix = f"encoder.{name}.{idx}."
    sd = RC.make_state(101, 1, 1)
    stride = 2 if prefix + "downsample.0.weight" in sd else 1
    Co, Ci = sd[prefix + "conv1.weight"].shape[:2]
    g = torch.Generator().manual_seed(Co + idx)
    x = torch.randn(6, Ci, 8, 8, generator=g).to(torch.bfloat16).float()
    gout = torch.randn(6, Co, 8 // stride, 8 // stride, generator=g)
    run = lambda ref, xl: [ref.block(xl, prefix, stride)]
    want = stage_grads(sd, prefix, x, [gout], run, torch.float64, None)
    drift = stage_grads(sd, prefix, x, [gout], run, torch.float32, torch.bfloat16)
    anchor = {k: rel_l2(drift[k], want[k]) for k in want}
    m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=1).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.unfreeze_encoder(name).train()
    blk = getattr(m.encoder, name)[idx]
    xd = RC.nhwc(x).to(torch.bfloat16).to(DEV).requires_grad_(True)
    a = m._block(xd, blk, [], True)
    (a.float() * RC.nhwc(gout).to(DEV)).sum().backward()
    ops.join_forward_side(xd.device)
    torch.cuda.synchronize()
    got = {"x": RC.nchw(xd.grad.float().cpu())}
    got.update({prefix + k: p.grad.cpu() for k, p in blk.named_parameters()})
    report(f"block {name}.{idx}", got, want, anchor)


def test_stem_pool_and_first_layer_against_f64():
    """The stem (the 7x7 weight gradient over the saved im2col matrix), the pooling backward with the skip gradient added inside,
    and layer1 behind it: gradients of sum(f1*g1) + sum(f2*g2) for every tensor of conv1 / bn1 / layer1."""
    sd = RC.make_state(101, 1, 1)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 2, 2, 32, 32, generator=g)
    g1, g2 = torch.randn(6, 64, 16, 16, generator=g), torch.randn(6, 64, 8, 8, generator=g)
    tm = lambda t: t.transpose(0, 1).reshape(6, *t.shape[2:])                 # the model's image order is t*B + b
    run = lambda ref, xl: ref.encoder(xl)[:2]
    names = lambda d: {k: v for k, v in d.items() if k.startswith(("encoder.conv1.", "encoder.bn1.", "encoder.layer1."))}
    want = names(stage_grads(sd, "encoder.", tm(x), [g1, g2], run, torch.float64, None))
    drift = names(stage_grads(sd, "encoder.", tm(x), [g1, g2], run, torch.float32, torch.bfloat16))
    assert len(want) == 3 + 12 and all(v is not None for v in want.values())
    anchor = {k: rel_l2(drift[k], want[k]) for k in want}
    m = U.PretrainedTemporalUNet(out_channels=1, lstm_layers=1).to(DEV)
    m.load_state_dict(sd, strict=True)
    m.unfreeze_encoder(("stem", "layer1")).train()
    pending = []
    feats = m._encode(x.to(DEV), pending, 0)
    (feats[0].float() * RC.nhwc(g1).to(DEV)).sum().add((feats[1].float() * RC.nhwc(g2).to(DEV)).sum()).backward()
    ops.join_forward_side(torch.device(DEV))
    torch.cuda.synchronize()
    got = {"encoder." + k: p.grad.cpu() for k, p in m.encoder.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    report("stem + pool + layer1", got, want, anchor)
