"""tests/optim_cases.py checked without a GPU: the f64 references against torch.optim.AdamW / clip_grad_norm_ in f64, the
loss-scale transitions against a hand-written table, the counted bounds against a plain f32 evaluation of the header's formulas
(inside every bound on every case table) and against six wrong evaluations (each outside on some case), the case tables'
own claims, and the argument validation of the optimiser's C ABI that returns before any launch (what
tests/test_param_groups_host.py covers for uclstm_adamw_step_groups is not repeated)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optim_cases as OC
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd.optim import check_run_table

F = np.float32
MUTANTS = ("bc_step_minus_1", "eps_inside_sqrt", "decay_on_gradient", "clip_without_min", "group_off_by_one", "f32_exp2_bias_correction")


def emulate(p, m, v, g, sumsq, max_norm, hyper, step, scale=None, mutant=None):
    """The update in numpy f32, one rounding per operation, pow in f64 for the bias corrections (rounded once).  `hyper` =
    (lr, b1, b2, eps, wd), scalars or per-element arrays.  `mutant` names one deliberate mistake."""
    lr, b1, b2, eps, wd = (np.asarray(a, dtype=F) for a in hyper)
    one = F(1.0)
    with np.errstate(all="ignore"):
        def clip_factor(total):
            q = F(max_norm) / (total + F(1e-6))
            return q if mutant == "clip_without_min" else np.minimum(q, one)
        if scale is None:
            coef = one
            if sumsq is not None and max_norm > 0:
                coef = clip_factor(F(np.sqrt(np.float64(sumsq))))
        else:
            inv = one / F(scale)
            coef = inv
            if max_norm > 0:
                coef = inv * clip_factor(F(np.sqrt(np.float64(sumsq))) * inv)
        t = step - 1 if mutant == "bc_step_minus_1" else step
        if mutant == "f32_exp2_bias_correction":
            inv_bc1 = one / (one - np.exp2(F(t) * np.log2(b1)))
            inv_sqrt_bc2 = one / np.sqrt(one - np.exp2(F(t) * np.log2(b2)))
        else:
            inv_bc1 = (1.0 / (1.0 - np.power(b1.astype(np.float64), float(t)))).astype(F)
            inv_sqrt_bc2 = (1.0 / np.sqrt(1.0 - np.power(b2.astype(np.float64), float(t)))).astype(F)
        gi = g * coef
        if mutant == "decay_on_gradient":
            gi = gi + wd * p
            w = p
        else:
            w = p * (one - lr * wd)
        mi = b1 * m + (one - b1) * gi
        vi = b2 * v + ((one - b2) * gi) * gi
        if mutant == "eps_inside_sqrt":
            denom = np.sqrt(vi + eps) * inv_sqrt_bc2
        else:
            denom = np.sqrt(vi) * inv_sqrt_bc2 + eps
        w = w - lr * inv_bc1 * mi / denom
    assert w.dtype == F and mi.dtype == F and vi.dtype == F
    return w, mi, vi


def worst_ratio(got, ref):
    """max over p, m, v and elements of |err| / bound (0 / 0 counts as inside, anything non-finite as outside)."""
    worst = 0.0
    for x, r, b in zip(got, ref[:3], ref[3:]):
        d = np.abs(x.astype(np.float64) - r)
        if not np.all(np.isfinite(d)):
            return float("inf")
        ratio = np.divide(d, b, out=np.where(d > 0, np.inf, 0.0), where=b > 0)
        worst = max(worst, float(ratio.max()))
    return worst


def single_case_ratio(case, mutant=None, scale=None):
    name, n, h, step, (_, sumsq, max_norm), first = case
    p, m, v, g = OC.make_inputs(n, seed=step + 13 * h, first_step=first)
    hyper = OC.HYPER_SETS[h]
    if scale is not None:
        if sumsq is None:
            sumsq, max_norm = 4.0, 0.0                       # the scaled forms need *sumsq: no clipping is max_norm <= 0
        g, sumsq = (g * F(scale)).astype(F), sumsq * scale * scale
    coef, rel = OC.clip_coef_ref(sumsq, max_norm, scale)
    ref = OC.adamw_ref(p, m, v, g, coef, *hyper, step, rel)
    return worst_ratio(emulate(p, m, v, g, sumsq, max_norm, hyper, step, scale, mutant), ref)


def table_case_ratio(case, mutant=None, step=3):
    name, n, runs, ng = case
    p, m, v, g = OC.make_inputs(n, seed=len(runs), first_step=False)
    _, sumsq, max_norm = OC.CLIP_X50
    coef, rel = OC.clip_coef_ref(sumsq, max_norm)
    ref = OC.groups_ref(p, m, v, g, coef, runs, ng, step, rel)
    grp = OC.group_index(runs, n)
    if mutant == "group_off_by_one":                         # element i looked up as element i + 1
        grp = np.concatenate((grp[1:], grp[-1:]))
    return worst_ratio(emulate(p, m, v, g, sumsq, max_norm, OC.group_hypers(grp, ng), step, None, mutant), ref)


@functools.lru_cache(maxsize=None)
def table_cases():
    return OC.run_table_cases()


# ---------------------------------------------------------------------------------------------
# the references are what torch computes in f64
# ---------------------------------------------------------------------------------------------
def _torch_steps(p0, grads, groups_of, hypers, max_norm, steps):
    """`steps` steps of clip_grad_norm_ + torch.optim.AdamW in f64 on the CPU; one tensor per group."""
    idx = [np.nonzero(groups_of == k)[0] for k in range(len(hypers))]
    params = [torch.nn.Parameter(torch.tensor(p0[i], dtype=torch.float64)) for i in idx]
    opt = torch.optim.AdamW([{"params": [q], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3], "weight_decay": h[4]}
                             for q, h in zip(params, hypers)])
    for s in range(steps):
        for q, i in zip(params, idx):
            q.grad = torch.tensor(grads[s][i], dtype=torch.float64)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
    out = np.empty_like(p0, dtype=np.float64)
    m, v = np.empty_like(out), np.empty_like(out)
    for q, i in zip(params, idx):
        out[i], m[i], v[i] = q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy()
    return out, m, v


def _rel(a, b):
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1e-300)))


@pytest.mark.parametrize("max_norm", [None, 1.0, 1e6])
@pytest.mark.parametrize("h", [0, 1, 2, 4, 6])
def test_adamw_ref_and_clip_coef_ref_equal_torch_adamw_in_f64_over_five_steps(h, max_norm):
    rng = np.random.default_rng(h)
    n, hyper = 300, OC.HYPER_SETS[h]
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 3.0 for _ in range(5)]
    want = _torch_steps(p0, grads, np.zeros(n, dtype=np.int64), [hyper], max_norm, 5)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for s in range(5):
        coef, _ = OC.clip_coef_ref(float((grads[s] ** 2).sum()), max_norm) if max_norm is not None else OC.clip_coef_ref(None, 0.0)
        assert (coef < 0.1) if max_norm == 1.0 else (coef == 1.0)
        p, m, v, *_ = OC.adamw_ref(p, m, v, grads[s], coef, *hyper, s + 1)
    assert max(_rel(p, want[0]), _rel(m, want[1]), _rel(v, want[2])) <= 1e-12


def test_groups_ref_equals_torch_adamw_over_parameter_groups_in_f64():
    rng = np.random.default_rng(77)
    n, ng = 2 * OC.CHUNK + 37, 5
    b = [0, 3, 700, 1024, 1500, 1501, n]
    runs = np.array([(b[i], b[i + 1], (2 * i) % ng) for i in range(len(b) - 1)], dtype=np.int64)
    check_run_table(runs.tolist(), n, ng)
    grp = OC.group_index(runs, n)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) for _ in range(5)]
    want = _torch_steps(p0, grads, grp, [OC.HYPER_SETS[k % 8] for k in range(ng)], 1.0, 5)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for s in range(5):
        coef, _ = OC.clip_coef_ref(float((grads[s] ** 2).sum()), 1.0)
        p, m, v, *_ = OC.groups_ref(p, m, v, grads[s], coef, runs, ng, s + 1)
    assert max(_rel(p, want[0]), _rel(m, want[1]), _rel(v, want[2])) <= 1e-12


def test_clip_coef_ref_cases():
    assert OC.clip_coef_ref(None, 1.0) == (1.0, 0.0) and OC.clip_coef_ref(4.0, 0.0) == (1.0, 0.0) == OC.clip_coef_ref(4.0, -1.0)
    assert OC.clip_coef_ref(0.25, 1.0) == (1.0, 0.0) and OC.clip_coef_ref(0.0, 1.0) == (1.0, 0.0)
    c, rel = OC.clip_coef_ref(2500.0, 1.0)
    assert abs(c - 1.0 / (50.0 + 1e-6)) < 1e-15 and rel == 3 * OC.U32
    assert OC.clip_coef_ref(4.0, 0.0, 1024.0) == (2.0 ** -10, OC.U32)
    c, rel = OC.clip_coef_ref(2500.0 * 2.0 ** 20, 1.0, 1024.0)                  # *sumsq of the scaled gradients
    assert abs(c * 1024.0 - 1.0 / (50.0 + 1e-6)) < 1e-15 and rel == 7 * OC.U32
    assert OC.clip_coef_ref(0.25 * 2.0 ** 20, 1.0, 1024.0) == (2.0 ** -10, OC.U32)


def test_loss_scale_update_ref_follows_the_hand_written_transition_table():
    for state, ss, gr, bo, it, want in OC.LOSS_SCALE_TABLE:
        assert OC.loss_scale_update_ref(state, ss, gr, bo, it) == want, (state, ss, gr, bo, it)
    s = [64.0, 0.0, 0.0]
    for ss, want in zip(OC.LOSS_SCALE_WALK, OC.LOSS_SCALE_WALK_STATES):
        s = OC.loss_scale_update_ref(s, ss, 2.0, 0.5, 2)
        assert s == want


# ---------------------------------------------------------------------------------------------
# the bounds are attainable, and they bite
# ---------------------------------------------------------------------------------------------
def test_f32_emulation_lies_inside_every_bound_of_the_single_group_matrix():
    worst = 0.0
    for case in OC.single_group_cases():
        for scale in (None,) + OC.SCALES:
            r = single_case_ratio(case, scale=scale)
            assert r <= 1.0, (case[0], scale, r)
            worst = max(worst, r)
    for n in OC.SINGLE_N:
        r = single_case_ratio((f"n{n}", n, OC.HYPER_MODEL, 3, OC.CLIP_X50, False))
        assert r <= 1.0, (n, r)
        worst = max(worst, r)
    print(f"[bounds] f32 emulation, single-group matrix: worst |err| / bound {worst:.3f}")
    assert worst > 0.05                                      # the bounds are within a small factor of what f32 really does


def test_f32_emulation_lies_inside_every_bound_of_the_run_table_cases():
    for case in table_cases():
        r = table_case_ratio(case)
        assert r <= 1.0, (case[0], r)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_each_mutant_of_the_emulation_falls_outside_a_bound(mutant):
    if mutant == "group_off_by_one":
        ratios = [table_case_ratio(c, mutant) for c in table_cases() if c[1] <= 5 * OC.CHUNK and len(c[2]) > 1]
    else:
        ratios = [single_case_ratio(c, mutant) for c in OC.single_group_cases()]
    print(f"[bounds] mutant {mutant}: outside on {sum(r > 1.0 for r in ratios)} of {len(ratios)} cases, worst {max(ratios):.3g} x the bound")
    assert max(ratios) > 1.0


def test_the_f32_exp2_bias_correction_is_outside_at_the_early_steps_and_inside_late():
    """Finding 1 of the issue, as modelled with correctly rounded f32 log2 / exp2: 1 - 0.999^t loses up to 8.9e-6 relative at
    small t, several times the counted bound of an update on p == 0; at t = 1000 the cancellation is gone."""
    early = [single_case_ratio((f"t{t}", 257, OC.HYPER_MODEL, t, OC.CLIP_X50, True), "f32_exp2_bias_correction") for t in (1, 2, 3, 4)]
    assert max(early) > 2.0, early


# ---------------------------------------------------------------------------------------------
# the case tables are what they claim to be
# ---------------------------------------------------------------------------------------------
def test_every_run_table_is_one_the_kernel_may_walk_and_reaches_its_path():
    cases = table_cases()                                    # the reach assertions run inside run_table_cases()
    for name, n, runs, ng in cases:
        assert runs.dtype == np.int64 and runs.shape[1] == 3
        check_run_table(runs.tolist(), n, ng)
        assert 1 <= ng <= OC.MAX_GROUPS and len(OC.group_index(runs, n)) == n
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    assert max(c[1] for c in cases) == OC.GROUPS_SWEEP + OC.CHUNK + 5          # the largest buffer: 2.1 M floats


def test_single_group_matrix_covers_the_required_cases():
    cases = OC.single_group_cases()
    assert {c[3] for c in cases} == set(OC.STEPS) | {OC.BIG_STEP}
    assert {c[2] for c in cases} >= {OC.HYPER_MODEL, OC.HYPER_WD0, OC.HYPER_B1_0, OC.HYPER_LR0}
    assert {c[4][0] for c in cases} == {c[0] for c in OC.CLIP_CASES} and {c[5] for c in cases} == {True, False}
    h = OC.HYPER_SETS
    assert h[OC.HYPER_WD0][4] == 0 and h[OC.HYPER_B1_0][1] == 0 and h[OC.HYPER_LR0][0] == 0
    assert 1.0 - h[0][1] ** OC.BIG_STEP == 1.0 and 1.0 - h[0][2] ** OC.BIG_STEP == 1.0
    p, m, v, g = OC.make_inputs(257, 0, False)
    assert ((g == 0) & (v != 0)).any() and ((g == 0) & (v == 0) & (m == 0)).any() and ((p == 0) & (g != 0)).any() and ((p == 0) & (g == 0)).any()
    assert not OC.make_inputs(257, 0, True)[1].any() and not OC.make_inputs(257, 0, True)[2].any()
    assert OC.SINGLE_N[-1] == 2048 * 256 + 257


# ---------------------------------------------------------------------------------------------
# argument validation at the C ABI: every call returns before any launch (host pointers, never dereferenced)
# ---------------------------------------------------------------------------------------------
def _host_pointers():
    buf = (C.c_float * 64)()
    assert C.addressof(buf) % 16 == 0
    return buf, C.cast(buf, C.c_void_p), C.c_void_p(C.addressof(buf) + 4)


def test_loss_scale_update_validates_before_any_launch():
    buf, p, _ = _host_pointers()
    f = L.lib.uclstm_loss_scale_update
    for args in ((None, p, 2.0, 0.5, 2000), (p, None, 2.0, 0.5, 2000), (p, p, 0.5, 0.5, 2000), (p, p, 2.0, 0.0, 2000), (p, p, 2.0, -0.5, 2000),
                 (p, p, 2.0, 1.5, 2000), (p, p, 2.0, 0.5, 0), (p, p, 2.0, 0.5, -3)):
        assert f(*args, None) == -1, args


def test_single_group_step_entry_points_validate_before_any_launch():
    buf, p, p4 = _host_pointers()
    step = L.lib.uclstm_adamw_step
    for bad_step in (0, -1):
        assert step(p, p, p, p, 64, None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, bad_step, None) == -1
    for i in range(4):
        args = [p, p, p, p]
        args[i] = None
        assert step(*args, 64, None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1, None) == -1
        assert L.lib.uclstm_adamw_step_dev(*args, 64, None, p, None) == -1
        assert L.lib.uclstm_adamw_step_scaled(*args, 64, p, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, p, None) == -1
    assert step(p, p, p, p, 0, None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1, None) == -1
    assert L.lib.uclstm_adamw_step_dev(p, p, p, p, 64, None, p4, None) == -1                       # hyper not 16-byte aligned
    assert L.lib.uclstm_adamw_step_dev(p, p, p, p, 64, None, None, None) == -1
    assert L.lib.uclstm_adamw_step_scaled(p, p, p, p, 64, None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, p, None) == -1      # sumsq required
    assert L.lib.uclstm_adamw_step_scaled(p, p, p, p, 64, p, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-4, None, None) == -1
