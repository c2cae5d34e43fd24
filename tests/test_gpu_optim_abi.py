"""The optimiser family of csrc/loss_optim.hip -- uclstm_adamw_step, uclstm_adamw_step_dev, uclstm_adamw_step_scaled,
uclstm_adamw_step_groups (with and without scale_state) and uclstm_loss_scale_update -- each called directly at the C ABI and
compared with the f64 references of tests/optim_cases.py on the same f32 inputs, at EVERY element of p, m and v.

The tests that went before reach these kernels through FusedAdamW at one friendly size, compare them with an f32 oracle or with
each other at 1e-5 .. 2e-5, look at p alone, and never leave the first trip of a loop.  Here *sumsq is a chosen f64 value (the
clip coefficient is controlled), the sizes are the smallest that reach every path (1, 255, 256, 257, 2048*256 + 257 elements; run
tables with boundaries on, next to and between the lanes' elements of a 1024-element chunk, 300 runs in one chunk, a second trip at
element 2 097 152 over 5000 table rows, 4097 runs, 257 and 1024 groups), and the bounds are counted per f32 operation
(optim_cases.py, module docstring; u = 2^-24):
  m'   2u |b1 m| + (3u + e_g) |(1-b1) g coef|                        e_g = u + the clip coefficient's own 0 / 3u / u / 7u
  v'   2u b2 v + (4u + 2 e_g) (1-b2) (g coef)^2
  p'   u |p'| + ~3u |decay p| + |U| (4u + err_denom / denom) + bound_m lr / (bc1 denom),  U the update,
       err_denom = A (3u + bound_v / (2 v')) + u denom,  A = sqrt(v' / bc2);  all three times 1 + 2^-10 (second order)
Checks that need no tolerance are bit-exact: the group lookup (a multi-group launch equals the element-wise selection from
one-group launches over the whole buffer), one run and one group against uclstm_adamw_step_dev (no state) and against
uclstm_adamw_step_scaled (with state), lr = 0 leaves p alone, a norm below max_norm gives the m', v' of a launch without clipping,
an overflowed step writes nothing, the device-side counters move by exactly one, uclstm_loss_scale_update's transitions.
Buffers carry eight guard elements behind their end, checked after every launch.

Measured on MI355X: worst |err| / bound over all 104 tests of this file (p / m / v):
  uclstm_adamw_step            0.549 / 0.971 / 0.966        uclstm_adamw_step_dev                       0.549 / 0.971 / 0.966
  uclstm_adamw_step_scaled     0.549 / 0.969 / 0.958        uclstm_adamw_step_groups, no scale_state    0.678 / 0.973 / 0.992
  uclstm_adamw_step_groups with scale_state   0.678 / 0.973 / 0.992      (m and v sit close to 1: where one term dominates,
  their bounds are two roundings, and among a million elements some have both near half a unit.  Every bit-exact check holds.)
Before its bias corrections were formed in double, uclstm_adamw_step_scaled (1 - exp2f(t * log2f(beta)) in f32) measured
p 0.53 at step 1, 4.89 / 4.77 / 4.59 at steps 2 / 3 / 4 and 0.51 / 0.53 at steps 10 / 1000, against 0.53 / 0.51 / 0.50 / 0.51 now;
with *sumsq = 1e301 both scaled entry points skipped the step and uclstm_loss_scale_update counted it.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optim_cases as OC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import _lib as L
    from unet_convlstm_amd import ops

DEV = "cuda"
F = np.float32
GUARD = 8
ENTRIES = ("step", "dev", "scaled", "groups", "groups_state")
SCALED_ENTRIES = ("scaled", "groups_state")
SECOND_TRIP_N = OC.GROUPS_SWEEP + OC.CHUNK + 5
WORST = {}                                                   # (entry, output) -> worst |err| / bound seen in this session


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    L.check(getattr(L.lib, name)(*args, ops._stream()), name)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def to_dev(a, offset):
    """`a` on the device, beginning `offset` elements into its allocation (offset 1: 4-byte alignment only), with GUARD
    sentinel elements behind it."""
    t = torch.full((offset + len(a) + GUARD,), -7.25, dtype=torch.float32, device=DEV)
    t[offset:offset + len(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t, t[offset:offset + len(a)]


def launch(entry, arrs, sumsq, max_norm, hyper, step, scale=None, runs=None, n_groups=1, offset=0):
    """One launch of an entry point on copies of (p, m, v, g); returns the new p, m, v as numpy.  `hyper` = (lr, b1, b2, eps, wd),
    or None with a run table: group k then uses OC.HYPER_SETS[k % 8].  The bias-correction step `step` goes in as the entry
    point takes it: an argument, hyper[6] + 1, hyper[1] + 1 or scale_state[2] + 1.  Asserted on every launch: the guard elements
    and g are untouched; uclstm_adamw_step_dev moves hyper[6] by exactly 1 and leaves hyper[0..5] and [7] alone;
    uclstm_adamw_step_groups moves hyper[1] by exactly 1 without scale_state and leaves the table alone with it; scale_state is
    never written by a step kernel."""
    n = len(arrs[0])
    full, view = zip(*(to_dev(a, offset) for a in arrs))
    p, m, v, g = view
    ss = None if sumsq is None else torch.tensor([sumsq], dtype=torch.float64, device=DEV)
    state = state0 = None
    if entry in SCALED_ENTRIES:
        assert ss is not None and scale is not None
        state = torch.tensor([scale, 5.0, step - 1], dtype=torch.float32, device=DEV)
        state0 = state.cpu().numpy().copy()
    if entry == "step":
        call("uclstm_adamw_step", ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(ss), max_norm, *hyper, step)
    elif entry == "dev":
        h = torch.tensor([*hyper, max_norm, step - 1, 42.0], dtype=torch.float32, device=DEV)
        h0 = h.cpu().numpy().copy()
        call("uclstm_adamw_step_dev", ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(ss), ptr(h))
        h1 = h.cpu().numpy()
        assert same_bits(h1[:6], h0[:6]) and h1[7] == h0[7] and h1[6] == h0[6] + 1.0, (h0, h1)
    elif entry == "scaled":
        call("uclstm_adamw_step_scaled", ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(ss), max_norm, *hyper, ptr(state))
    else:
        if runs is None:
            runs = np.array([[0, n, 0]], dtype=np.int64)
        rows = [hyper] if hyper is not None else [OC.HYPER_SETS[k % 8] for k in range(n_groups)]
        assert len(rows) == n_groups
        table = np.zeros((1 + n_groups, 8), dtype=F)
        table[0, 0], table[0, 1] = max_norm, (step - 1 if entry == "groups" else 77.0)
        table[0, 2:] = 3.5                                   # reserved: must survive
        table[1:, :5] = np.array(rows, dtype=F)
        table[1:, 5:] = -2.5
        h = torch.from_numpy(table).to(DEV)
        r = torch.from_numpy(np.ascontiguousarray(runs, dtype=np.int64)).to(DEV)
        call("uclstm_adamw_step_groups", ptr(p), ptr(m), ptr(v), ptr(g), n, ptr(ss), ptr(r), int(runs.shape[0]), ptr(h), n_groups, ptr(state))
        h1 = h.cpu().numpy()
        want = table.copy()
        if entry == "groups":
            want[0, 1] += 1.0
        assert same_bits(h1, want), "the hyper table: only hyper[1] may move, by exactly 1, and only without scale_state"
    out = tuple(t.cpu().numpy() for t in (p, m, v))
    if state is not None:
        assert same_bits(state.cpu().numpy(), state0), "a step kernel wrote scale_state"
    assert same_bits(g.cpu().numpy(), np.ascontiguousarray(arrs[3])), "g was written"
    for t in full:
        edge = torch.cat((t[:offset], t[offset + n:])).cpu().numpy()
        assert bool((edge == F(-7.25)).all()), "a write outside [0, n)"
    return out


def scaled_problem(entry, arrs, sumsq, max_norm, scale):
    """The same problem as an entry point sees it: the scaled ones get g * scale, *sumsq * scale^2 (both exact: scale is a power
    of two) and need *sumsq, so `no clipping` is max_norm <= 0 there.  Returns (arrs, sumsq, max_norm, scale or None)."""
    if entry not in SCALED_ENTRIES:
        return arrs, sumsq, max_norm, None
    if sumsq is None:
        sumsq, max_norm = 4.0, 0.0
    p, m, v, g = arrs
    gs = (g * F(scale)).astype(F)
    assert bool(np.array_equal(gs.astype(np.float64), g.astype(np.float64) * scale))
    return (p, m, v, gs), sumsq * scale * scale, max_norm, scale


def ratios(got, ref):
    """worst |err| / bound of p, m, v over every element (non-finite output: inf; an error where the bound is 0: inf)."""
    out = []
    for x, r, b in zip(got, ref[:3], ref[3:]):
        x = x.astype(np.float64)
        if x.shape != r.shape or not bool(np.isfinite(x).all()):
            out.append(float("inf"))
            continue
        d = np.abs(x - r)
        out.append(float(np.divide(d, b, out=np.where(d > 0, np.inf, 0.0), where=b > 0).max()))
    return out


def note(entry, rs):
    for name, r in zip("pmv", rs):
        WORST[(entry, name)] = max(WORST.get((entry, name), 0.0), r)


def report(what, entry, worst, count):
    print(f"[parity] {what} [{entry}]: worst |err| / bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f} (<= 1) over {count} launches;"
          f" session worst p {WORST[(entry, 'p')]:.3f} m {WORST[(entry, 'm')]:.3f} v {WORST[(entry, 'v')]:.3f}")


def run_and_check(entry, arrs, sumsq, max_norm, hyper, step, scale=1024.0, **kw):
    """Launch, compare with adamw_ref / groups_ref inside the counted bounds; returns (outputs, ratios)."""
    a, ss, mx, sc = scaled_problem(entry, arrs, sumsq, max_norm, scale)
    got = launch(entry, a, ss, mx, hyper, step, scale=sc, **kw)
    coef, rel = OC.clip_coef_ref(ss, mx, sc)
    if kw.get("runs") is not None and hyper is None:
        ref = OC.groups_ref(*a, coef, kw["runs"], kw["n_groups"], step, rel)
    else:
        ref = OC.adamw_ref(*a, coef, *hyper, step, rel)
    rs = ratios(got, ref)
    note(entry, rs)
    return got, rs


# ---------------------------------------------------------------------------------------------
# 1. every entry point against adamw_ref
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_hyper_sets_steps_clip_cases_and_specials_against_f64(entry):
    """The matrix of OC.single_group_cases(): hyper sets x steps 1, 2, 3, 4, 10, 1000, 100000 at a norm 50 x max_norm, every clip
    case at the model's own set, each at m = v = 0 and with a state, on 257 elements with the planted specials."""
    worst, kept, count = [0.0, 0.0, 0.0], {}, 0
    for name, n, h, step, (clip, sumsq, max_norm), first in OC.single_group_cases():
        arrs = OC.make_inputs(n, seed=step + 13 * h, first_step=first)
        got, rs = run_and_check(entry, arrs, sumsq, max_norm, OC.HYPER_SETS[h], step)
        assert max(rs) <= 1.0, f"{entry} {name}: |err| / bound p {rs[0]:.3f} m {rs[1]:.3f} v {rs[2]:.3f}"
        worst = [max(a, b) for a, b in zip(worst, rs)]
        count += 1
        if h == OC.HYPER_LR0:
            assert same_bits(got[0], arrs[0]), f"{entry} {name}: lr = 0 must leave p bit-identical"
        if h == OC.HYPER_MODEL and step == 2:
            kept[(clip, first)] = got
        i = np.arange(n) % 11
        if first:                                            # g == 0 with m == v == 0: the update is 0, m' and v' stay 0
            assert not got[1][i == 4].any() and not got[2][i == 4].any()
    for first in (True, False):                              # a norm below max_norm: the coefficient is exactly 1
        for clip in ("below", "zero", "max_norm_0", "max_norm_neg"):
            assert same_bits(kept[(clip, first)][1], kept[("null", first)][1]) and same_bits(kept[(clip, first)][2], kept[("null", first)][2]), \
                f"{entry} {clip}: m', v' differ from those of the launch without clipping"
            assert same_bits(kept[(clip, first)][0], kept[("null", first)][0])
    report("hyper sets x steps x clip cases, n = 257", entry, worst, count)


@pytest.mark.parametrize("n,offset", [(n, 0) for n in OC.SINGLE_N] + [(257, 1)], ids=lambda x: str(x))
@pytest.mark.parametrize("entry", ENTRIES)
def test_element_counts_and_a_four_byte_aligned_buffer_against_f64(entry, n, offset):
    arrs = OC.make_inputs(n, seed=offset, first_step=False)
    _, sumsq, max_norm = OC.CLIP_X50
    _, rs = run_and_check(entry, arrs, sumsq, max_norm, OC.HYPER_SETS[OC.HYPER_MODEL], 3, offset=offset)
    report(f"n = {n}, buffers {4 if offset else 16}-byte aligned", entry, rs, 1)
    assert max(rs) <= 1.0


@pytest.mark.parametrize("entry", ENTRIES)
def test_five_consecutive_steps_each_against_f64_from_the_kernels_own_state(entry):
    n, worst = 1025, [0.0, 0.0, 0.0]
    p, m, v, _ = OC.make_inputs(n, seed=5, first_step=True)
    _, sumsq, max_norm = OC.CLIP_X50
    for step in range(1, 6):
        g = OC.make_inputs(n, seed=50 + step, first_step=True)[3]
        (p2, m2, v2), rs = run_and_check(entry, (p, m, v, g), sumsq, max_norm, OC.HYPER_SETS[OC.HYPER_MODEL], step)
        assert max(rs) <= 1.0, (entry, step, rs)
        assert not same_bits(p2, p) and not same_bits(m2, m)
        worst = [max(a, b) for a, b in zip(worst, rs)]
        p, m, v = p2, m2, v2
    report("five consecutive steps, n = 1025", entry, worst, 5)


# ---------------------------------------------------------------------------------------------
# 2. the run table of uclstm_adamw_step_groups
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_cases():
    return OC.run_table_cases()


def table_case_ids():
    return [c[0] for c in OC.run_table_cases()]


@pytest.mark.parametrize("entry", ["groups", "groups_state"])
@pytest.mark.parametrize("name", table_case_ids())
def test_run_table_walk_is_bit_exact_and_within_the_bounds(name, entry):
    """A multi-group launch equals, bit for bit in p, m and v, the element-wise selection by each element's group from one-run,
    one-group launches over copies of the whole buffer (one per distinct hyper set, same *sumsq): the same instructions run per
    element and contraction is pinned off in that kernel.  Then the multi-group result against groups_ref."""
    _, n, runs, ng = next(c for c in table_cases() if c[0] == name)
    U.optim.check_run_table(runs.tolist(), n, ng)            # the caller's duty before any launch (uclstm.h)
    arrs = OC.make_inputs(n, seed=len(runs), first_step=False)
    _, sumsq, max_norm = OC.CLIP_X50
    a, ss, mx, sc = scaled_problem(entry, arrs, sumsq, max_norm, 1024.0)
    got, rs = run_and_check(entry, arrs, sumsq, max_norm, None, 3, runs=runs, n_groups=ng)
    sets = OC.group_index(runs, n) % 8
    want = [np.full(n, np.nan, dtype=F) for _ in range(3)]
    for s in sorted(set(sets.tolist())):
        one = launch(entry, a, ss, mx, OC.HYPER_SETS[s], 3, scale=sc)
        for w, o in zip(want, one):
            w[sets == s] = o[sets == s]
    for nm, x, w in zip("pmv", got, want):
        bad = np.nonzero(bits(x) != bits(w))[0]
        assert bad.size == 0, f"{name} [{entry}] {nm}: {bad.size} elements differ from the one-group launch of their group, first at {bad[:5]}"
    report(f"run table {name}: n = {n}, {len(runs)} runs, {ng} groups, selection bit-exact", entry, rs, 1)
    assert max(rs) <= 1.0


@pytest.mark.parametrize("n", OC.SINGLE_N + (1023, 1025, SECOND_TRIP_N))
def test_one_run_one_group_equals_the_single_group_entry_points_bit_for_bit(n):
    """uclstm.h: without scale_state uclstm_adamw_step_groups equals uclstm_adamw_step_dev bit for bit, with it
    uclstm_adamw_step_scaled -- at every element count of this file, the second trips of both loops included."""
    arrs = OC.make_inputs(n, seed=n % 97, first_step=False)
    h = OC.HYPER_SETS[OC.HYPER_MODEL]
    for clip, sumsq, max_norm in (OC.CLIP_X50, OC.CLIP_CASES[0]):
        dev, grp = (launch(e, arrs, sumsq, max_norm, h, 4) for e in ("dev", "groups"))
        assert all(same_bits(a, b) for a, b in zip(dev, grp)), f"n = {n}, clip {clip}: groups != step_dev"
        a, ss, mx, sc = scaled_problem("scaled", arrs, sumsq, max_norm, 1024.0)
        sca, gst = (launch(e, a, ss, mx, h, 4, scale=sc) for e in SCALED_ENTRIES)
        assert all(same_bits(a_, b_) for a_, b_ in zip(sca, gst)), f"n = {n}, clip {clip}: groups with scale_state != step_scaled"
    print(f"[parity] one run, one group, n = {n}: groups == step_dev and groups with scale_state == step_scaled bit for bit")


# ---------------------------------------------------------------------------------------------
# 3. loss scaling
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", OC.SCALES)
@pytest.mark.parametrize("entry", SCALED_ENTRIES)
def test_scaled_entry_points_on_g_times_scale_stay_within_the_bounds_of_adamw_ref_on_g(entry, scale):
    """Steps 1, 2, 3, 4, 10, 1000 taken from scale_state[2], at m = v = 0 and with a state, clipped and not.  A bias correction
    formed in f32 as 1 - exp2(t log2 beta) leaves the bound of p at the early steps (optim_cases' host test shows the model);
    both entry points form it in double."""
    worst, count = [0.0, 0.0, 0.0], 0
    for step in OC.STEPS:
        for first in (True, False):
            for _, sumsq, max_norm in (OC.CLIP_X50, OC.CLIP_CASES[1]):
                arrs = OC.make_inputs(1025, seed=step, first_step=first)
                got, rs = run_and_check(entry, arrs, sumsq, max_norm, OC.HYPER_SETS[OC.HYPER_MODEL], step, scale=scale)
                assert max(rs) <= 1.0, f"{entry} scale {scale} step {step} first {first} max_norm {max_norm}: p {rs[0]:.3f} m {rs[1]:.3f} v {rs[2]:.3f}"
                worst = [max(a, b) for a, b in zip(worst, rs)]
                count += 1
    report(f"scale {scale:g}, steps {OC.STEPS}", entry, worst, count)


def scale_update(state, sumsq, growth=2.0, backoff=0.5, interval=2000):
    st = torch.tensor(state, dtype=torch.float32, device=DEV)
    ss = torch.tensor([sumsq], dtype=torch.float64, device=DEV)
    call("uclstm_loss_scale_update", ptr(st), ptr(ss), growth, backoff, interval)
    return [float(x) for x in st.cpu().numpy()], float(ss.item())


@pytest.mark.parametrize("sumsq", [float("inf"), float("nan"), float("-inf")], ids=["inf", "nan", "-inf"])
@pytest.mark.parametrize("entry", SCALED_ENTRIES)
def test_an_overflowed_step_writes_nothing_and_the_scale_backs_off(entry, sumsq):
    for n in (257, OC.SWEEP + 257):
        arrs = OC.make_inputs(n, seed=9, first_step=False)
        for max_norm in (1.0, 0.0):
            got = launch(entry, arrs, sumsq, max_norm, OC.HYPER_SETS[OC.HYPER_MODEL], 3, scale=1024.0)
            assert all(same_bits(x, a) for x, a in zip(got, arrs[:3])), f"{entry}: *sumsq = {sumsq} wrote p, m or v"
    after, ss = scale_update([1024.0, 5.0, 2.0], sumsq)
    assert after == [512.0, 0.0, 2.0] == OC.loss_scale_update_ref([1024.0, 5.0, 2.0], sumsq, 2.0, 0.5, 2000)


@pytest.mark.parametrize("entry", SCALED_ENTRIES)
def test_step_kernels_and_loss_scale_update_agree_about_a_huge_finite_sumsq(entry):
    """*sumsq = 1e301 (not reachable from f32 gradients, finite all the same): skipped and backed off, or applied and counted --
    never skipped and counted.  The header says applied: the step is then also held to adamw_ref."""
    arrs = OC.make_inputs(1025, seed=11, first_step=False)
    a, ss, mx, sc = scaled_problem(entry, arrs, 4.0, 0.0, 1024.0)
    got = launch(entry, a, 1e301, mx, OC.HYPER_SETS[OC.HYPER_MODEL], 3, scale=sc)
    applied = not all(same_bits(x, y) for x, y in zip(got, arrs[:3]))
    after, _ = scale_update([1024.0, 5.0, 2.0], 1e301)
    counted, backed_off = after[2] == 3.0, after[0] == 512.0
    print(f"[parity] *sumsq = 1e301 [{entry}]: step applied {applied}, counted {counted}, scale backed off {backed_off}")
    assert counted != backed_off and applied == counted, "a step was skipped and counted (or applied and backed off)"
    assert not OC.step_overflowed(1e301) and applied and after == OC.loss_scale_update_ref([1024.0, 5.0, 2.0], 1e301, 2.0, 0.5, 2000)
    coef, rel = OC.clip_coef_ref(1e301, mx, sc)
    rs = ratios(got, OC.adamw_ref(*a, coef, *OC.HYPER_SETS[OC.HYPER_MODEL], 3, rel))
    assert max(rs) <= 1.0, rs


def test_loss_scale_update_walks_the_transition_table_exactly():
    for state, sumsq, growth, backoff, interval, want in OC.LOSS_SCALE_TABLE:
        after, ss = scale_update(state, sumsq, growth, backoff, interval)
        assert after == want, (state, sumsq, growth, backoff, interval, after)
        assert ss == sumsq or (ss != ss and sumsq != sumsq)                     # *sumsq is read only
    st = torch.tensor([64.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    for sumsq, want in zip(OC.LOSS_SCALE_WALK, OC.LOSS_SCALE_WALK_STATES):     # ten steps on ONE device state
        ss = torch.tensor([sumsq], dtype=torch.float64, device=DEV)
        call("uclstm_loss_scale_update", ptr(st), ptr(ss), 2.0, 0.5, 2)
        assert [float(x) for x in st.cpu().numpy()] == want, (sumsq, want)
    print(f"[parity] uclstm_loss_scale_update: {len(OC.LOSS_SCALE_TABLE)} transitions and a ten-step walk, exact")


@pytest.mark.parametrize("route", ["eager", "groups", "capturable"])
def test_steps_done_counts_only_the_successful_steps_with_loss_scaling(route):
    """good, overflowed, good: every loss-scaling route reports 2, and so does state_dict()["fused"]["step"]."""
    torch.manual_seed(3)
    a, b = (torch.nn.Parameter(torch.randn(s, device=DEV)) for s in (300, 41))
    if route == "eager":
        opt = U.FusedAdamW([a, b], lr=1e-3, max_grad_norm=1.0, loss_scale=1024.0)
        assert not opt.uses_groups and not opt.capturable
    elif route == "groups":
        opt = U.FusedAdamW([{"params": [a]}, {"params": [b], "weight_decay": 0.0}], lr=1e-3, max_grad_norm=1.0, loss_scale=1024.0)
        assert opt.uses_groups and len(opt.param_groups) == 2
    else:
        opt = U.FusedAdamW([a, b], lr=1e-3, max_grad_norm=1.0, loss_scale=1024.0, capturable=True)
        assert opt.uses_groups and opt.capturable
    before = opt.flat.flat_p.clone()
    for k, poison in enumerate((False, True, False)):
        opt.flat.flat_g.copy_(torch.randn(opt.flat.numel, device=DEV) * 1024.0)
        if poison:
            opt.flat.flat_g[17] = float("inf")
            held = opt.flat.flat_p.clone()
        opt.step()
        if poison:
            assert torch.equal(opt.flat.flat_p, held)
    assert not torch.equal(opt.flat.flat_p, before)
    assert opt.scale_state.tolist() == [512.0, 1.0, 2.0]
    assert opt.steps_done() == 2 and opt.state_dict()["fused"]["step"] == 2
