"""Fine-tuning on the fast path (GPU): FusedAdamW with parameter groups against torch.optim.AdamW, the one-sweep kernel
uclstm_adamw_step_groups against its single-group neighbours, loss scaling inside it, the graphed fp16 step, frozen weights in
the operators' backward passes, checkpoints and FlatDDP with a frozen weight."""
import collections
import ctypes as C

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops

DEV = "cuda"

SHAPES = [(7, 3), (5,), (4, 2, 3, 3), (1,), (64,), (16, 8, 3, 3)]
GROUP_OF = [0, 1, 0, 1, 1, 2]
GROUP_CFG = [dict(lr=1e-3, weight_decay=1e-4), dict(lr=1e-3, weight_decay=0.0), dict(lr=2.5e-4, weight_decay=1e-2, betas=(0.8, 0.99))]


def _groups(params):
    return [dict(params=[p for p, g in zip(params, GROUP_OF) if g == k], **cfg) for k, cfg in enumerate(GROUP_CFG)]


def _case(seed=11):
    """Six tensors, eight gradients each: steps 1 and 5 large (the clip is active), the others small."""
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * (3.0 if step in (1, 5) else 0.05) for s in SHAPES] for step in range(1, 9)]
    return init, grads


def _fused(init, **kw):
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = U.FusedAdamW(_groups(ps), max_grad_norm=1.0, order=ps, **kw)
    return ps, opt


def _fused_step(ps, opt, grads):
    opt.zero_grad()
    for p, g in zip(ps, grads):
        p.grad.copy_(g)
    opt.step()


@pytest.mark.parametrize("capturable", [False, True])
def test_interleaved_groups_match_torch_adamw_with_a_global_clip(capturable):
    """Three INTERLEAVED groups (own lr / weight decay / betas), one global clip_grad_norm_(1.0), group 2's lr halved before
    step 4 (ReduceLROnPlateau), eight steps, against clip_grad_norm_ + torch.optim.AdamW(groups) in f32 on the CPU."""
    init, grads = _case()
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    ropt = torch.optim.AdamW(_groups(ref))
    ps, opt = _fused(init, capturable=capturable)
    assert opt.uses_groups and opt.runs.tolist() == [[0, 21, 0], [21, 26, 1], [26, 98, 0], [98, 163, 1], [163, 1315, 2]]
    for step in range(1, 9):
        if step == 4:
            for o in (ropt, opt):
                o.param_groups[2]["lr"] *= 0.5
        for p, g in zip(ref, grads[step - 1]):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        ropt.step()
        _fused_step(ps, opt, grads[step - 1])
        torch.testing.assert_close(opt.grad_norm().float().cpu().reshape(()), total.float().reshape(()), rtol=1e-5, atol=1e-6)
        worst = max(float((p.detach().cpu() - r.detach()).abs().max()) for p, r in zip(ps, ref))
        print(f"[parity] groups vs torch.optim.AdamW (capturable={capturable}) step {step}: norm {float(total):.5f}, max |dp| {worst:.2e}")
        for p, r in zip(ps, ref):
            torch.testing.assert_close(p.detach().cpu(), r.detach(), rtol=1e-5, atol=1e-6)
    assert opt.steps_done() == 8 and opt.state_dict()["fused"]["step"] == 8
    with pytest.raises(RuntimeError, match="add_param_group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, device=DEV))]})


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_one_group_through_the_groups_entry_point_is_the_device_hyper_kernel_bit_for_bit():
    torch.manual_seed(3)
    n = 10007
    p0 = torch.randn(n, device=DEV)
    gs = [torch.randn(n, device=DEV) * s for s in (2.0, 0.01, 0.3)]
    lr, b1, b2, eps, wd, mx = 1e-2, 0.9, 0.999, 1e-8, 1e-4, 1.0
    res = []
    for groups in (False, True):
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sq = torch.zeros(1, dtype=torch.float64, device=DEV)
        if groups:
            hyper = torch.tensor([[mx, 0, 0, 0, 0, 0, 0, 0], [lr, b1, b2, eps, wd, 0, 0, 0]], dtype=torch.float32, device=DEV)
            runs = torch.tensor([[0, n, 0]], dtype=torch.int64, device=DEV)
        else:
            hyper = torch.tensor([lr, b1, b2, eps, wd, mx, 0, 0], dtype=torch.float32, device=DEV)
        for g in gs:
            sq.zero_()
            L.check(L.lib.uclstm_sumsq(_ptr(g), n, _ptr(sq), None), "sumsq")
            if groups:
                L.check(L.lib.uclstm_adamw_step_groups(_ptr(p), _ptr(m), _ptr(v), _ptr(g), n, _ptr(sq), _ptr(runs), 1, _ptr(hyper), 1, None,
                                                       None), "adamw_step_groups")
            else:
                L.check(L.lib.uclstm_adamw_step_dev(_ptr(p), _ptr(m), _ptr(v), _ptr(g), n, _ptr(sq), _ptr(hyper), None), "adamw_step_dev")
        torch.cuda.synchronize()
        res.append((p, m, v, float(hyper[0, 1] if groups else hyper[6])))
    (pa, ma, va, ca), (pb, mb, vb, cb) = res
    assert not torch.equal(pa, p0)
    assert torch.equal(pb, pa) and torch.equal(mb, ma) and torch.equal(vb, va) and ca == cb == 3.0


def test_loss_scaling_in_the_groups_kernel_equals_the_plain_update_and_skips_overflowed_steps():
    """The scenario of test_gpu_fp16.test_loss_scaled_adamw_equals_plain_adamw_and_skips_overflowed_steps through
    uclstm_adamw_step_groups with two groups (three runs, one of a single element)."""
    torch.manual_seed(73)
    n = 10007
    p0, g0 = torch.randn(n, device=DEV), torch.randn(n, device=DEV) * 1e-3
    runs = torch.tensor([[0, 4001, 0], [4001, 4002, 1], [4002, n, 0]], dtype=torch.int64, device=DEV)

    def run(scaled, g, steps=3):
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        sq = torch.zeros(1, dtype=torch.float64, device=DEV)
        state = torch.tensor([1024.0, 0.0, 0.0], device=DEV)
        grp = [1e-2, 0.9, 0.999, 1e-8, 1e-4, 0, 0, 0]
        hyper = torch.tensor([[0.01, 0, 0, 0, 0, 0, 0, 0], grp, grp], dtype=torch.float32, device=DEV)
        for s in range(1, steps + 1):
            sq.zero_()
            gg = g * state[0] if scaled else g
            L.check(L.lib.uclstm_sumsq(_ptr(gg), n, _ptr(sq), None), "sumsq")
            if scaled:
                L.check(L.lib.uclstm_adamw_step_groups(_ptr(p), _ptr(m), _ptr(v), _ptr(gg), n, _ptr(sq), _ptr(runs), 3, _ptr(hyper), 2,
                                                       _ptr(state), None), "adamw_step_groups")
                L.check(L.lib.uclstm_loss_scale_update(_ptr(state), _ptr(sq), 2.0, 0.5, 2, None), "scale_update")
            else:
                L.check(L.lib.uclstm_adamw_step(_ptr(p), _ptr(m), _ptr(v), _ptr(gg), n, _ptr(sq), 0.01, 1e-2, 0.9, 0.999, 1e-8, 1e-4, s, None),
                        "adamw")
        torch.cuda.synchronize()
        return p, m, v, state, hyper
    pa = run(False, g0)[0]
    pb, _, _, st, hy = run(True, g0)
    print(f"[parity] loss-scaled groups kernel vs plain AdamW: max |dp| {float((pb - pa).abs().max()):.2e}")
    torch.testing.assert_close(pb, pa, rtol=2e-5, atol=2e-6)
    assert st.tolist() == [2048.0, 1.0, 3.0]              # grew once after two good steps in a row, three successful steps
    assert float(hy[0, 1]) == 0.0                         # with loss scaling the count is scale_state[2], not the global block's
    bad = g0.clone()
    bad[5] = float("inf")
    pc, mc, vc, st, _ = run(True, bad, steps=2)
    assert torch.equal(pc, p0) and not bool(mc.any()) and not bool(vc.any())
    assert st.tolist() == [256.0, 0.0, 0.0]               # both steps skipped, scale halved twice, no successful step


def _decay_groups(model, **kw):
    ps = [p for p in model.parameters() if p.requires_grad]
    return [dict(params=[p for p in ps if p.ndim > 1], weight_decay=1e-4, **kw), dict(params=[p for p in ps if p.ndim <= 1], weight_decay=0.0, **kw)]


def test_graphed_fp16_step_with_groups_replays_the_eager_step_and_skips_an_overflow():
    """GraphedTrainStep under compute_dtype(float16): two groups (decay / no decay), loss_scale 2**14, capturable.  A replay and
    an eager step from the SAME state agree: loss to 1e-6 relative, parameters rel-L2 <= 1e-5 -- the criterion of
    test_graphed_train_step_replays_the_eager_step for bf16 -- unless two EAGER fp16 steps from that state (measured here, printed)
    already differ by more, in which case the bound is twice that figure (two independent draws of the same noise).  Then a
    replay whose target holds one inf: parameters and both moments unchanged, scale halved, successful-step count unmoved, all
    decided on the device."""
    def make():
        torch.manual_seed(5)
        m = U.TemporalUNetDualView(1, 1, base_ch=64, use_skip_lstm=True).to(DEV).train()
        o = U.FusedAdamW(_decay_groups(m), lr=1e-3, max_grad_norm=1.0, loss_scale=2.0 ** 14, capturable=True, order=m.parameters())
        return m, o

    def same_state(m_to, o_to, m_from, o_from):
        m_to.load_state_dict(m_from.state_dict())
        o_to.m.copy_(o_from.m)
        o_to.v.copy_(o_from.v)
        o_to.scale_state.copy_(o_from.scale_state)
        o_to.group_hyper.copy_(o_from.group_hyper)
        assert torch.equal(o_to.flat.flat_p, o_from.flat.flat_p)

    d = U.SyntheticSequences(4, 3, 64, 64, seed=6, kind="uniform")
    with ops.compute_dtype(torch.float16):
        m1, o1 = make()
        m2, o2 = make()
        m3, o3 = make()
        assert o2.uses_groups and o2.runs.shape[0] > 40          # BatchNorm / bias tensors interleave with the weights
        g = U.GraphedTrainStep(m2, o2, d.x, d.y, d.mask, True, warmup=2)
        assert o2.scale_state.tolist() == [2.0 ** 14, 2.0, 2.0]  # two eager warm-up steps, none overflowed; the capture ran nothing
        same_state(m1, o1, m2, o2)
        same_state(m3, o3, m2, o2)
        l1, _ = U.train_step(m1, o1, d.x, d.y, d.mask, True)
        l3, _ = U.train_step(m3, o3, d.x, d.y, d.mask, True)
        l2, yp = g(d.x, d.y, d.mask)
        torch.cuda.synchronize()
        e_ee = rel_l2(o3.flat.flat_p.cpu(), o1.flat.flat_p.cpu())
        e_p = rel_l2(o2.flat.flat_p.cpu(), o1.flat.flat_p.cpu())
        bound = 1e-5 if e_ee <= 1e-5 else 2.0 * e_ee
        print(f"[parity] fp16 graph replay vs eager step from the same state: loss {float(l2):.7f} / {float(l1):.7f} (eager again "
              f"{float(l3):.7f}), parameters rel-L2 {e_p:.2e}; eager vs eager {e_ee:.2e}; bound {bound:.2e}; grad norm "
              f"{float(o2.grad_norm()):.5f} / {float(o1.grad_norm()):.5f}")
        assert abs(float(l2) - float(l1)) <= 1e-6 * abs(float(l1)) and e_p <= bound and yp.shape[1] == 3
        assert o2.scale_state.tolist() == [2.0 ** 14, 3.0, 3.0] and o2.steps_done() == 3
        assert abs(float(o2.grad_norm()) - float(o1.grad_norm())) <= 1e-3 * float(o1.grad_norm())
        # an overflowed step THROUGH the graph: the forward pass and the BatchNorm buffers depend on x only and stay finite
        p, m, v = o2.flat.flat_p.clone(), o2.m.clone(), o2.v.clone()
        y_bad = d.y.clone()
        y_bad[0, 0, 0, 0, 0] = float("inf")
        l_bad, _ = g(d.x, y_bad, d.mask)
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(l_bad)) and not bool(torch.isfinite(o2.sumsq).all())
        assert torch.equal(o2.flat.flat_p, p) and torch.equal(o2.m, m) and torch.equal(o2.v, v)
        assert o2.scale_state.tolist() == [2.0 ** 13, 0.0, 3.0] and o2.steps_done() == 3
        # and the next good replay trains again
        l_ok, _ = g(d.x, d.y, d.mask)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(l_ok)) and not torch.equal(o2.flat.flat_p, p) and o2.scale_state.tolist() == [2.0 ** 13, 1.0, 4.0]


LSTM_WEIGHTS = ("temporal.layers.0.conv.weight", "lstm_skip3.layers.0.conv.weight", "lstm_skip2.layers.0.conv.weight")


def _one_step(frozen, base=64, B=4, T=3, hw=64, out_ch=1):
    """One bf16 train_step of the skip-LSTM model from seed 5 with ``frozen`` parameters' requires_grad off.  Returns
    (launch log, {name: gradient}, {name: parameter before}, {name: parameter after})."""
    torch.manual_seed(5)
    model = U.TemporalUNetDualView(1, out_ch, base_ch=base, use_skip_lstm=True).to(DEV).train()
    named = dict(model.named_parameters())
    for k in frozen:
        named[k].requires_grad_(False)
    before = {k: p.detach().clone() for k, p in named.items()}
    opt = U.FusedAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    d = U.SyntheticSequences(B, T, hw, hw, seed=6, kind="uniform")
    y, mask = (t.expand(-1, -1, out_ch, -1, -1).contiguous() for t in (d.y, d.mask))
    ops.LAUNCH_LOG = []
    try:
        U.train_step(model, opt, d.x, y, mask, True)
        torch.cuda.synchronize()
        log = list(ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
    grads = {k: (None if k in frozen else p.grad.detach().clone()) for k, p in named.items()}
    after = {k: p.detach().clone() for k, p in named.items()}
    return log, grads, before, after


def _wgrad_diff(log_all, log_frozen):
    """(N, Ktot) of the weight-gradient launches the frozen run lacks; everything else must be the same sequence."""
    wa = collections.Counter(e for e in log_all if e[0] == "wgrad")
    wf = collections.Counter(e for e in log_frozen if e[0] == "wgrad")
    assert not (wf - wa), f"the frozen run launched weight-gradient GEMMs the all-trainable run did not: {wf - wa}"
    assert [e for e in log_all if e[0] != "wgrad"] == [e for e in log_frozen if e[0] != "wgrad"]      # forward / input gradients
    return sorted((e[2], e[3]) for e in (wa - wf).elements())


def _lstm_keys(base):
    return sorted((int(d.N), int(d.Ktot)) for d in (ops.lstm_wgrad_unpack_desc(hd, hd, 3) for hd in (16 * base, 8 * base, 4 * base)))


def _frozen_untouched(run, frozen):
    _, grads, before, after = run
    for k in frozen:
        assert grads[k] is None and torch.equal(after[k], before[k]), k
    moved = [k for k in grads if k not in frozen and not torch.equal(after[k], before[k])]
    assert len(moved) >= (len(grads) - len(frozen)) // 2
    assert any(float(g.abs().max()) > 0 for g in grads.values() if g is not None)


# The yardstick shape of the frozen-weight test.  At every shape of the one-output-channel model two all-trainable runs
# differ (measured on MI355X: (base_ch 8, B 1, T 2, 32 x 32), (8, 1, 1, 32), (8, 2, 2, 32), (8, 1, 2, 64), (16, 1, 2, 32) all
# differ in outc.conv.weight / outc.conv.bias, the larger ones also in inc.net.0.weight): the fused output head adds one f32
# atomic per block of the BatchNorm reduction, and that reduction has a block per 32 pixel rows.  With TWO output channels the
# head is the stand-alone 1x1 kernel, which at <= 2048 pixels finishes with at most two atomics per element (commutative from
# a zeroed buffer), and the bias column sums run in one block.
EXACT = dict(base=8, B=1, T=2, hw=32, out_ch=2)


def test_frozen_convlstm_weights_launch_no_weight_gradient_and_leave_the_others_alone():
    """The three ConvLSTM gate weights frozen (their biases stay trainable).

    Launches, at base_ch 64, B 4, T 3, 64 x 64 (the model of the graphed-step test, bf16): the frozen run has exactly the three
    ConvLSTM weight-gradient GEMMs fewer (identified by N, Ktot) and the same forward / input-gradient launches; frozen weights get
    no gradient and do not move.

    Gradients: "equal to the all-trainable run" is decided by a yardstick the frozen path has no part in, the all-trainable step
    run twice from the same state.  This is the torch.equal variant: at EXACT (see above; a smaller model with two output
    channels) two all-trainable runs are bit-identical, asserted here first, and the frozen run must then be torch.equal to
    them in every trainable gradient.  At base_ch 64 the run-to-run figures (atomics in the bias column sums and the fused
    head, 0 .. 9e-7 per tensor) are printed next to the frozen run's, without a bound: single-draw noise of a one-element
    tensor is no yardstick.

    Second case: down1's first convolution weight frozen, its BatchNorm affine trainable -- dgamma and dbeta still arrive and
    match (torch.equal at EXACT)."""
    conv = ("down1.net.1.net.0.weight",)
    # launch sequence at the size of the graphed-step test
    a, b, frz = _one_step(()), _one_step(()), _one_step(LSTM_WEIGHTS)
    gone = _wgrad_diff(a[0], frz[0])
    print(f"[parity] frozen ConvLSTM weights at base_ch 64: {len([e for e in a[0] if e[0] == 'wgrad'])} -> "
          f"{len([e for e in frz[0] if e[0] == 'wgrad'])} weight-gradient launches, gone (N, Ktot) {gone}")
    assert gone == _lstm_keys(64) and len(gone) == 3
    assert a[0] == b[0]
    _frozen_untouched(frz, LSTM_WEIGHTS)
    for k, g in frz[1].items():
        if g is not None:
            e, noise = rel_l2(g, a[1][k]), rel_l2(b[1][k], a[1][k])
            if e or noise:
                print(f"[parity] base_ch 64 {k}: frozen vs all-trainable rel-L2 {e:.3e}, all-trainable run to run {noise:.3e}")
            assert e <= 1e-5, k                       # the project's f32 tolerance; a wrong or missing gradient is O(1)
    frz = _one_step(conv)
    assert len(_wgrad_diff(a[0], frz[0])) == 1
    _frozen_untouched(frz, conv)
    # gradients, bit for bit, where the all-trainable step is reproducible
    a, b = _one_step((), **EXACT), _one_step((), **EXACT)
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), f"all-trainable runs differ in {k}: EXACT is no yardstick on this machine"
    for frozen in (LSTM_WEIGHTS, conv):
        frz = _one_step(frozen, **EXACT)
        gone = _wgrad_diff(a[0], frz[0])
        assert gone == (_lstm_keys(EXACT["base"]) if frozen is LSTM_WEIGHTS else gone[:1]) and len(gone) == len(frozen)
        _frozen_untouched(frz, frozen)
        for k, g in frz[1].items():
            if g is not None:
                assert torch.equal(g, a[1][k]), k
        trainable_partners = [k.replace("weight", "bias") for k in LSTM_WEIGHTS] if frozen is LSTM_WEIGHTS else \
            ["down1.net.1.net.1.weight", "down1.net.1.net.1.bias"]
        for k in trainable_partners:
            assert float(frz[1][k].abs().max()) > 0, k
    print(f"[parity] frozen vs all-trainable at {EXACT}: every trainable gradient bit-identical (all-trainable run to run: bit-identical)")


def test_checkpoint_round_trip_continues_bit_for_bit_and_refuses_another_grouping():
    init, grads = _case(seed=12)
    ps, opt = _fused(init)
    for step in range(3):
        _fused_step(ps, opt, grads[step])
    opt.param_groups[2]["lr"] *= 0.5
    sd = opt.state_dict()
    assert sd["fused"]["step"] == 3 and sd["fused"]["tensor_groups"] == GROUP_OF and len(sd["param_groups"]) == 3
    now = [p.detach().cpu().clone() for p in ps]
    _fused_step(ps, opt, grads[3])
    ps2, opt2 = _fused(now)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[2]["lr"] == opt.param_groups[2]["lr"] == 1.25e-4 and opt2.steps_done() == 3
    _fused_step(ps2, opt2, grads[3])
    torch.cuda.synchronize()
    for p, q in zip(ps, ps2):
        assert torch.equal(p, q)
    assert torch.equal(opt.m, opt2.m) and torch.equal(opt.v, opt2.v) and opt2.steps_done() == 4
    # another grouping of the same tensors (same group count, same numel)
    ps3 = [torch.nn.Parameter(t.clone().to(DEV)) for t in now]
    other = [0, 0, 1, 1, 1, 2]
    opt3 = U.FusedAdamW([dict(params=[p for p, g in zip(ps3, other) if g == k], **cfg) for k, cfg in enumerate(GROUP_CFG)], order=ps3)
    with pytest.raises(ValueError, match="grouping"):
        opt3.load_state_dict(sd)
    # a single-group state still loads into a single-group optimiser, and not into groups
    ps4 = [torch.nn.Parameter(t.clone().to(DEV)) for t in now]
    o4 = U.FusedAdamW(ps4, lr=1e-3)
    _fused_step(ps4, o4, grads[0])
    sd4 = o4.state_dict()
    old = {k: v for k, v in sd4["fused"].items() if k not in ("sizes", "tensor_groups")}          # as saved before groups existed
    o5 = U.FusedAdamW([torch.nn.Parameter(t.clone().to(DEV)) for t in now], lr=1e-3)
    o5.load_state_dict({**sd4, "fused": old})
    assert torch.equal(o5.m, o4.m) and o5.step_count == 1
    with pytest.raises(ValueError):
        opt3.load_state_dict({**sd4, "fused": old})


def test_flat_ddp_with_a_frozen_convlstm_weight_and_two_groups_launches_every_bucket_once():
    """One rank on the real RCCL backend (the pattern of test_flat_ddp_over_rccl_single_rank_matches_plain_training): a frozen
    weight is outside FlatParams, announces nothing, and no bucket waits for it -- every bucket is launched exactly once per
    step, and no more of them are left to finalize() than with every parameter trainable."""
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29678", rank=0, world_size=1, device_id=torch.device(DEV, 0))
        created = True
    try:
        data = U.SyntheticSequences(4, 3, 32, 32, seed=5, kind="blobs")

        def run(freeze):
            torch.manual_seed(77)
            model = U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV).train()
            weight = dict(model.named_parameters())["temporal.layers.0.conv.weight"]
            weight.requires_grad_(not freeze)
            w0 = weight.detach().clone()
            opt = U.FusedAdamW(_decay_groups(model), lr=1e-3, order=model.parameters())
            assert opt.uses_groups and any(p is weight for p in opt.flat.params) != freeze
            ddp = U.FlatDDP(model, opt.flat, bucket_mb=0.05)
            launched, late, in_finalize = collections.Counter(), [], [False]
            launch, finalize = ddp._launch, ddp.finalize

            def counting(bi):
                launched[bi] += 1
                if in_finalize[0]:
                    late.append(bi)
                launch(bi)

            def finalize_marked():
                in_finalize[0] = True
                try:
                    finalize()
                finally:
                    in_finalize[0] = False

            ddp._launch, ddp.finalize = counting, finalize_marked
            p0 = opt.flat.flat_p.clone()
            n_late = 0
            for _ in range(2):
                launched.clear()
                del late[:]
                loss, _ = U.train_step(model, opt, data.x, data.y, None, False, ddp)
                torch.cuda.synchronize()
                assert len(ddp.buckets) > 3 and sorted(launched) == list(range(len(ddp.buckets))) and set(launched.values()) == {1}
                assert bool(torch.isfinite(loss))
                n_late = max(n_late, len(late))
            assert not torch.equal(opt.flat.flat_p, p0)
            if freeze:
                assert torch.equal(weight, w0) and weight.grad is None
            ddp.remove_hooks()
            return len(ddp.buckets), n_late

        nb_all, late_all = run(False)
        nb_frz, late_frz = run(True)
        print(f"[parity] FlatDDP buckets left to finalize(): all trainable {late_all} of {nb_all}, frozen ConvLSTM weight {late_frz} of {nb_frz}")
        assert late_frz <= late_all
    finally:
        if created:
            dist.destroy_process_group()
