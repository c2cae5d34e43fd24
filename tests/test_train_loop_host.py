"""The helpers of tests/train_loop_cases.py on the CPU.

1. The negative control of the GPU test "each step against the oracle" has power: along the oracle's own trajectory at
   lr = 3e-3 a forward pass on the weights of the PREVIOUS step is at least 4 x the GPU test's bound (0.06 per-timestep rel-L2)
   away from the one on the live weights, at steps 2 and 3 of both fixtures, whereas the oracle's own bf16-storage drift on the
   same snapshots stays inside the bound the GPU test uses.  Measured with the f32 oracle: 0.109 .. 0.154 (model_noskip),
   0.178 .. 0.261 (model_skip); bf16-storage drift 0.008 .. 0.014.
2. ``oracle_trajectory`` is AdamW: the same gradients through ``torch.optim.AdamW`` give the same parameters over three steps.
3. ``PackSpy`` decides "hit" by the rule of ``ops.pack_weights``; ``first_difference`` names the tensor.
"""
import ctypes as C
import functools
import types

import pytest
import torch

import train_loop_cases as TL
from conftest import load_golden, sub
from oracle import unet_oracle as O

torch.set_num_threads(8)
FIXTURES = ["model_noskip", "model_skip"]


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """Computed once per fixture and shared, never modified."""
    g = load_golden(name)
    return g, TL.oracle_trajectory(sub(g, "p/"), g["x"], g["y"], g["mask"])


@pytest.mark.parametrize("name", FIXTURES)
def test_a_forward_pass_on_stale_weights_is_far_outside_the_bound(name):
    g, traj = trajectory(name)
    assert len(traj) == TL.ORACLE_STEPS == 3
    fresh = [s["y_pred"] for s in traj]
    stale = TL.stale_distances(fresh, fresh)
    for k, errs in zip((2, 3), stale):
        print(f"[train loop] {name} step {k}: f32 oracle, live against one-step-old weights, per-timestep rel-L2 {[round(e, 4) for e in errs]} "
              f"(required >= {TL.STALE_MIN})")
        assert min(errs) >= TL.STALE_MIN, f"{name} step {k}: {errs}"
    # the same separation as the GPU test sees it: the bf16-storage oracle on the previous snapshot against the f32 prediction,
    # and the drift of the bf16-storage oracle on the SAME snapshot, which the bound has to let through
    with torch.no_grad(), O.bf16_storage():
        emu = [torch.stack(O.model_forward(s["snapshot"], g["x"], None, True, {})[0], 1) for s in traj]
    for k in (1, 2, 3):
        drift = TL.per_t(emu[k - 1], fresh[k - 1])
        print(f"[train loop] {name} step {k}: bf16-storage oracle against the f32 oracle on the same snapshot {[round(e, 4) for e in drift]}")
        assert max(drift) <= 4e-2                        # tests/test_gpu_model.py: the inherent drift line
        if k > 1:
            far = TL.per_t(fresh[k - 1], emu[k - 2])
            assert min(far) >= TL.STALE_MIN and min(far) >= 3 * max(drift), f"{name} step {k}: stale {far}, drift {drift}"


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_trajectory_is_torch_adamw_on_the_same_gradients(name):
    """Bound: both sides are the same f32 formula in another order of operations -- a few roundings of 2^-24 on a parameter of
    magnitude |p| and on an update of at most lr: 2e-6 * |p| + 2e-7.  A wrong lr, decay, bias correction or clip is 1e-4 or more."""
    g, traj = trajectory(name)
    p0 = sub(g, "p/")
    names = [k for k in p0 if O.is_trainable(k)]
    params = [torch.nn.Parameter(p0[k].clone()) for k in names]
    opt = torch.optim.AdamW(params, lr=TL.LR, weight_decay=TL.WD)
    for k, s in enumerate(traj):
        for prm, key in zip(params, names):
            assert torch.equal(s["snapshot"][key], traj[k - 1]["after"][key] if k else p0[key])
            prm.grad = s["grads"][key].clone()
        torch.nn.utils.clip_grad_norm_(params, TL.CLIP)
        opt.step()
        moved = 0.0
        for prm, key in zip(params, names):
            torch.testing.assert_close(s["after"][key], prm.detach(), rtol=2e-6, atol=2e-7, msg=lambda m: f"{name} step {k + 1} {key}: {m}")
            moved = max(moved, float((s["after"][key] - s["snapshot"][key]).abs().max()))
        if k == 0:                                      # Adam's first step is lr * sign(g) (+ lr * wd * |p|): lr long, not the default 1e-3
            assert 0.99 * TL.LR <= moved <= 1.01 * TL.LR, moved


def test_oracle_train_step_keeps_its_defaults():
    g, _ = trajectory("model_noskip")
    p = sub(g, "p/")
    a = O.train_step(p, g["x"], g["y"], g["mask"], True)
    b = O.train_step(p, g["x"], g["y"], g["mask"], True, lr=1e-3, wd=1e-4)
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    torch.testing.assert_close(a[1]["outc.conv.weight"], sub(g, "p_after/")["outc.conv.weight"], rtol=1e-4, atol=1e-6)


class _Desc(C.Structure):
    _fields_ = [("N", C.c_int), ("Ktot", C.c_int)]


def _fake_ops():
    ops = types.SimpleNamespace(BF16=torch.bfloat16, _PACK_RECORDING=False, _PACK_READY={}, seen=[])

    def pack_weights(desc, w, elem_offset=0, dtype=torch.bfloat16, lookahead=True):
        ops.seen.append((elem_offset, dtype, lookahead))
        return torch.full((1,), float(len(ops.seen)))
    ops.pack_weights = pack_weights
    return ops


def test_pack_spy_counts_a_hit_by_the_rule_of_pack_weights():
    ops = _fake_ops()
    spy = TL.PackSpy(ops, keep_panels=True)
    d, w = _Desc(3, 5), torch.zeros(4)
    key = (w.data_ptr(), 2, bytes(d), torch.bfloat16)
    spy(d, w, 2)                                          # not recording: an in-line pack
    ops._PACK_RECORDING = True
    spy(d, w, 2)                                          # recording, the plan does not know the key
    ops._PACK_READY[key] = object()
    spy.step = 1
    out = spy(d, w, 2)                                    # a look-ahead panel
    spy(d, w, 2, lookahead=False)                         # a temporary: never from the plan
    spy(d, w, 3)                                          # another offset: another key
    spy(d, w, 2, torch.float16)                           # another dtype: another key
    assert [c[2] for c in spy.calls] == [False, False, True, False, False, False]
    assert spy.hits() == spy.hits(1) == 1 and spy.hits(0) == 0 and len(spy.misses(1)) == 2 and len(spy.misses(0)) == 2
    assert ops.seen[2:4] == [(2, torch.bfloat16, True), (2, torch.bfloat16, False)] and ops.seen[5][1] == torch.float16
    (step, d2, w2, off, dtype, panel), = spy.panels
    assert (step, off, dtype) == (1, 2, torch.bfloat16) and w2 is w and panel is out and bytes(d2) == bytes(d) and d2 is not d
    d.N = 7                                               # the spy kept a copy of the descriptor
    assert d2.N == 3


def test_first_difference_names_the_tensor_and_compares_bits():
    names, sizes = ["a.weight", "b.weight"], [3, 2]
    base = dict(loss=torch.tensor(1.0), flat_g=torch.arange(5.0), flat_p=torch.arange(5.0) + 1, m=torch.zeros(5), v=torch.ones(5))
    base["buffer bn.running_mean"] = torch.tensor([0.5, float("nan")])
    same = {k: v.clone() for k, v in base.items()}
    assert TL.first_difference(base, same, names, sizes) is None          # NaN in the same place is the same bits
    TL.compare("identical", base, same, names, sizes)
    other = {k: v.clone() for k, v in base.items()}
    other["flat_p"][4] += 1e-6
    other["v"][0] = 2.0
    assert TL.first_difference(base, other, names, sizes)[0] == "flat_p[b.weight]"
    with pytest.raises(AssertionError, match=r"flat_p\[b.weight\]"):
        TL.compare("changed", base, other, names, sizes)
    zero = {k: v.clone() for k, v in base.items()}
    zero["m"][1] = -0.0                                                    # equal as numbers, not as bits
    assert TL.first_difference(base, zero, names, sizes)[0] == "m[a.weight]"
    buf = {k: v.clone() for k, v in base.items()}
    buf["buffer bn.running_mean"][0] = 0.25
    assert TL.first_difference(base, buf, names, sizes)[0] == "buffer bn.running_mean"
