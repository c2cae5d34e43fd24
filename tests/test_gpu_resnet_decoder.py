"""The decoder of PretrainedTemporalUNet against f64, one DecoderBlock at a time and as a chain.

tests/test_gpu_resnet_model.py checks the decoder inside the whole model, where the model's own reduced-precision drift gives
per-tensor anchors of 0.4 .. 0.9: a gradient that is wrong by O(1) passes 2.5 x such an anchor.  One block on small inputs is not
chaotic -- the anchors here are a few per cent (tests/test_resnet_host.py caps them at 0.12 without a GPU) -- so a swapped K segment of
the two-source weight gradient, a skip gradient on the wrong tensor, a wrong ``c_valid``, a missing factor of the frozen-BatchNorm
backward or skips consumed in the wrong order stand out.  The yardstick is ``_Ref.decoder_block`` / ``_Ref.decoder`` of
tests/resnet_cases.py in f64 on the CPU; every tolerance is anchored in the drift of that same restatement in f32 under
``torch.autocast("cpu", dtype=<the test's dtype>)``:

  * gradients (x, skip, the block's six parameters): ``report`` = conftest.per_tensor_grad_report with its defaults, per tensor
    max(2.5 x anchor, 2e-2), the median ratio at most 1.25;
  * the block's output: rel-L2 <= max(1.25 x anchor, floor), floor 6e-3 in bf16 (the forward bound of one stage in
    tests/test_gpu_ops.py::test_conv_bn_relu_train_fwd_bwd_two_groups) and 6e-3 / 8 in fp16 (three more mantissa bits);
  * BatchNorm buffers: training mode through the same report and counters + 1 exactly, evaluation statistics bit-unchanged;
  * the backward launches per block: 2 weight-gradient GEMMs, 3 input-gradient GEMMs with a skip and 2 without.

BatchNorm runs in its three modes: batch statistics, running statistics with a backward pass (``model.eval()`` in grad mode: z is
kept and BatchNorm applied behind it) and running statistics under no_grad (scale and shift in the GEMM's epilogue; output only).
Inputs, references and anchors are computed once per case (RC.decoder_block_case / decoder_chain_case) and never modified.
Measured ratios and the kernel routes of every case are printed (run with -s) and recorded in profiles/resnet_decoder_parity.txt.
"""
import functools

import pytest
import torch

import resnet_cases as RC
from conftest import per_tensor_grad_report, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import modules, ops

DEV = "cuda"
torch.set_num_threads(16)
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
BLOCK_CASES = [pytest.param(i, shape, dtype, id=f"block{i}-n{shape[0]}-{shape[1]}x{shape[2]}-{NAME[dtype]}")
               for i in range(5) for shape in RC.decoder_block_shapes(i) for dtype in RC.DEC_DTYPES]


@functools.lru_cache(maxsize=None)
def model():
    """One model for the file; ``fresh`` puts the decoder and the head back to the seeded state before every run (the encoder and
    the ConvLSTMs are not run here)."""
    return U.PretrainedTemporalUNet(out_channels=1, lstm_layers=1).to(DEV)


def fresh(train):
    m, sd = model(), RC.decoder_state()
    m.decoder.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    m.head.load_state_dict({k[len("head."):]: v for k, v in sd.items() if k.startswith("head.")}, strict=True)
    for p in m.parameters():
        p.grad = None
    return m.train(train)


def to_dev(t, dtype, grad):
    """f32 NCHW values that ``dtype`` holds exactly -> the 16-bit NHWC tensor the model works on (every width here is a multiple of 8)."""
    return None if t is None else RC.nhwc(t).to(dtype).to(DEV).requires_grad_(grad)


def run(dtype, mode, inputs, gout, body):
    """``body(model, device inputs, pending)`` -> output, in BatchNorm mode ``mode`` ("train", "eval": running statistics with a
    backward pass, "no_grad": running statistics without), backward on sum(out * gout), then what ``forward`` does at its end.
    Host copies only: (output, input gradients by name, parameter gradients by short key, decoder buffers, log of forward, of backward)."""
    grad = mode != "no_grad"
    m = fresh(mode == "train")
    dev_in = {k: to_dev(v, dtype, grad) for k, v in inputs.items()}
    pending: list = []
    ops.LAUNCH_LOG = []
    try:
        with ops.compute_dtype(dtype), torch.set_grad_enabled(grad):
            out = body(m, dev_in, pending)
            n_fwd = len(ops.LAUNCH_LOG)
            if grad:
                g = gout.to(DEV) if out.dtype == torch.float32 else RC.nhwc(gout).to(DEV)
                (out.float() * g).sum().backward()
        modules._flush_counters(pending)
        ops.join_forward_side(dev_in["x"].device)
        torch.cuda.synchronize()
        log = list(ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
    out = out.detach().cpu() if out.dtype == torch.float32 else RC.nchw(out.detach().float().cpu())
    dx = {k: RC.nchw(v.grad.float().cpu()) for k, v in dev_in.items() if v is not None and v.grad is not None}
    dp = {"decoder." + k: p.grad.cpu() for k, p in m.decoder.named_parameters() if p.grad is not None}
    dp.update({"head." + k: p.grad.cpu() for k, p in m.head.named_parameters() if p.grad is not None})
    buffers = {k: v.cpu() for k, v in m.decoder.state_dict(prefix="decoder.").items() if RC.is_buffer(k)}
    return dict(out=out, dx=dx, dp=dp, buffers=buffers, log_f=log[:n_fwd], log_b=log[n_fwd:])


@functools.lru_cache(maxsize=None)
def block_run(i, shape, dtype, mode):
    ref = RC.decoder_block_case(i, shape, dtype, "eval" if mode == "no_grad" else mode)
    body = lambda m, d, pending: m._decoder_block(m.decoder.blocks[i], d["x"], d["skip"], pending)
    return run(dtype, mode, ref["inputs"], ref["gouts"][0], body)


@functools.lru_cache(maxsize=None)
def chain_run(dtype, mode):
    ref = RC.decoder_chain_case(dtype, mode)
    body = lambda m, d, pending: m._decode(d["x"], [d[f"skip{j}"] for j in range(4)] + [None], pending)
    return run(dtype, mode, ref["inputs"], ref["gouts"][0], body)


def routes(log):
    return "; ".join(repr(e) for e in log if e[0] in ("fwd", "wgrad"))


def check_output(what, got, ref, floor):
    e, anchor = rel_l2(got["out"], ref["out"]), ref["anchor_out"]
    bound = max(1.25 * anchor, floor)
    print(f"[parity] {what}: output rel-L2 {e:.6f}; anchor {anchor:.6f}, floor {floor:.6f}: bound {bound:.6f} "
          f"({'1.25 x anchor' if 1.25 * anchor >= floor else 'the floor'} decides), rel-L2 / bound {e / bound:.3f}, rel-L2 / anchor {e / anchor:.3f}; "
          f"forward launches: {routes(got['log_f'])}; backward launches: {routes(got['log_b'])}")
    assert tuple(got["out"].shape) == tuple(ref["out"].shape)
    assert e <= bound, f"{what}: output rel-L2 {e:.6f} > {bound:.6f}"


def check_buffers(what, got, ref, mode, moved):
    """Training mode: the running statistics under ``moved`` against the reference's through per_tensor_grad_report and their
    counters + 1; every other decoder buffer -- all of them with evaluation statistics -- bit-unchanged."""
    sd = RC.decoder_state()
    names = list(ref["anchor_buffers"])
    assert len(names) == (2 * moved if mode == "train" else 0) and (mode == "train" or not ref["buffers"])
    still = [k for k in got["buffers"] if k not in ref["buffers"]]
    assert len(still) + len(ref["buffers"]) == 30 and all(torch.equal(got["buffers"][k], sd[k]) for k in still), f"{what}: a buffer moved"
    if mode != "train":
        return
    counters = [k for k in ref["buffers"] if k.endswith("num_batches_tracked")]
    assert len(counters) == moved and all(int(got["buffers"][k]) == int(ref["buffers"][k]) == int(sd[k]) + 1 for k in counters)
    bad, rows, med = per_tensor_grad_report(names, got["buffers"], ref["buffers"], [float(ref["buffers"][k].double().norm()) for k in names],
                                            [ref["anchor_buffers"][k] for k in names])
    print(f"[parity] {what}: BatchNorm buffers: median rel-L2 / anchor {med:.3f} (bound 1.25); worst four (rel-L2 / bound): " +
          "; ".join(f"{k.split('.', 3)[-1]} {rel:.6f}/{bound:.6f}" for _, k, rel, bound, _, z in rows[:4] if not z))
    assert not bad, " | ".join(bad[:8])


def block_gradients(i, got):
    prefix = f"decoder.blocks.{i}."
    assert set(got["dp"]) == {prefix + k for k in ("conv1.0.weight", "conv1.1.weight", "conv1.1.bias", "conv2.0.weight", "conv2.1.weight",
                                                   "conv2.1.bias")}, sorted(got["dp"])
    return {**got["dx"], **got["dp"]}


@pytest.mark.parametrize("mode", RC.DEC_MODES)
@pytest.mark.parametrize("i,shape,dtype", BLOCK_CASES)
def test_one_decoder_block_against_f64(i, shape, dtype, mode):
    ref, got = RC.decoder_block_case(i, shape, dtype, mode), block_run(i, shape, dtype, mode)
    what = f"decoder block {i} n{shape[0]} {shape[1]}x{shape[2]} {NAME[dtype]} {mode}"
    has_skip = RC.DEC_SKIP[i] > 0
    assert set(ref["grads"]) == {"x"} | ({"skip"} if has_skip else set()) | {k for k in ref["sd"] if k.startswith(f"decoder.blocks.{i}.") and not RC.is_buffer(k)}
    assert set(got["dx"]) == ({"x", "skip"} if has_skip else {"x"})
    check_output(what, got, ref, RC.DEC_OUT_FLOOR[dtype])
    check_buffers(what, got, ref, mode, 2)
    # per block of the model test's 14 = 5 + 5 + 4 input-gradient GEMMs and 10 weight-gradient GEMMs
    assert not [e for e in got["log_f"] if e[0] == "wgrad"]
    assert len([e for e in got["log_b"] if e[0] == "wgrad"]) == 2
    assert len([e for e in got["log_b"] if e[0] == "fwd"]) == (3 if has_skip else 2)
    RC.report(what, block_gradients(i, got), ref["grads"], ref["anchor_grads"])


@pytest.mark.parametrize("i,shape,dtype", BLOCK_CASES)
def test_one_decoder_block_folded_epilogue_under_no_grad(i, shape, dtype):
    """Running statistics without a backward pass: BatchNorm's scale and shift in the GEMM's epilogue, one rounding per stage."""
    ref, got = RC.decoder_block_case(i, shape, dtype, "eval"), block_run(i, shape, dtype, "no_grad")
    what = f"decoder block {i} n{shape[0]} {shape[1]}x{shape[2]} {NAME[dtype]} no_grad"
    check_output(what, got, ref, RC.DEC_OUT_FLOOR[dtype])
    assert not [e for e in got["log_f"] + got["log_b"] if e[0] in ("wgrad", "reduce")]
    assert len([e for e in got["log_f"] if e[0] == "fwd"]) == 2 and not got["log_b"] and not got["dx"] and not got["dp"]
    check_buffers(what, got, ref, "no_grad", 0)


@pytest.mark.parametrize("mode", RC.DEC_MODES)
@pytest.mark.parametrize("dtype", RC.DEC_DTYPES, ids=lambda d: NAME[d])
def test_decoder_chain_against_f64(dtype, mode):
    """``_decode`` at the model's smallest decoder shapes (n = 4, 512 x 2 x 2 up to [4, 1, 64, 64]) against ``_Ref.decoder``.

    Through ten BatchNorm stages the per-tensor anchors of the chain are weak (0.15 .. 0.28 in bf16 on the CPU; the host test caps
    them at 0.30), so the per-tensor gradient check here is no sharper than the model test's.  The sharp parts are the bound on the
    f32 output, 1.25 x an anchor of about 0.01 with no floor, and that each of the four skips is compared with the gradient that
    belongs to it: skips consumed in another order, or a gradient handed to another skip, is O(1) in both."""
    ref, got = RC.decoder_chain_case(dtype, mode), chain_run(dtype, mode)
    what = f"decoder chain n{RC.DEC_CHAIN_N} {NAME[dtype]} {mode}"
    assert got["out"].dtype == torch.float32 and tuple(got["out"].shape) == (RC.DEC_CHAIN_N, 1, 64, 64)
    check_output(what, got, ref, 0.0)
    check_buffers(what, got, ref, mode, 10)
    assert set(got["dx"]) == {"x", "skip0", "skip1", "skip2", "skip3"}
    names = {k for k in ref["sd"] if not RC.is_buffer(k)}
    assert set(got["dp"]) == names and len(names) == 30 + 2 and set(ref["grads"]) == names | set(got["dx"])
    assert len([e for e in got["log_b"] if e[0] == "wgrad"]) == 10 and len([e for e in got["log_b"] if e[0] == "fwd"]) == 14
    RC.report(what, {**got["dx"], **got["dp"]}, ref["grads"], ref["anchor_grads"], label=lambda k: k.replace("decoder.blocks.", "blocks."))


class _SkipFirstRef(RC._Ref):
    """A deliberately WRONG restatement: cat([skip, x]) where smp has cat([x, skip])."""

    def concat(self, up, skip):
        return torch.cat([skip, up], 1)


@pytest.mark.parametrize("shape", RC.decoder_block_shapes(3), ids=lambda s: f"n{s[0]}-{s[1]}x{s[2]}")
def test_wrong_references_are_rejected(shape):
    """The tests above can fail: block 3, whose two sources both have 64 channels so that the wrong wirings keep every shape, in bf16
    and training mode.  The same GPU result that passes against the reference is rejected against (a) the reference with the concat
    the other way round -- what a swapped K segment, a skip gradient on the wrong tensor or a wrong ``c_valid`` order would look
    like -- and (b) the reference with the gradients of the two BatchNorm weights exchanged.  The wrong arithmetic is on the CPU side."""
    i, dtype = 3, torch.bfloat16
    ref, got = RC.decoder_block_case(i, shape, dtype, "train"), block_run(i, shape, dtype, "train")
    grads = block_gradients(i, got)
    RC.report(f"decoder block {i} n{shape[0]} against the reference", grads, ref["grads"], ref["anchor_grads"])
    wrong = RC.decoder_block_reference(i, shape, dtype, "train", ref_cls=_SkipFirstRef)
    assert set(wrong["grads"]) == set(ref["grads"]) and all(wrong["grads"][k].shape == ref["grads"][k].shape for k in ref["grads"])
    with pytest.raises(AssertionError, match="rel-L2"):
        RC.report(f"decoder block {i} n{shape[0]} against cat([skip, x])", grads, wrong["grads"], ref["anchor_grads"])
    with pytest.raises(AssertionError, match="output rel-L2"):
        check_output(f"decoder block {i} n{shape[0]} against cat([skip, x])", got, wrong, RC.DEC_OUT_FLOOR[dtype])
    g1, g2 = f"decoder.blocks.{i}.conv1.1.weight", f"decoder.blocks.{i}.conv2.1.weight"
    swapped = {**ref["grads"], g1: ref["grads"][g2], g2: ref["grads"][g1]}
    with pytest.raises(AssertionError, match="rel-L2"):
        RC.report(f"decoder block {i} n{shape[0]} against exchanged BatchNorm weight gradients", grads, swapped, ref["anchor_grads"])
