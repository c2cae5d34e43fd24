"""Helpers of tests/test_gpu_recurrence.py that need no GPU: the case table, the f64 references of ONE step of the ConvLSTM
recurrence (forward and backward) and of what follows the backward loop, and the bounds.  tests/test_recurrence_cases_host.py
pins the references, chained without rounding, to f64 autograd through F.conv2d, runs an f32 emulation of the device plan through
the same comparison and shows that wrong recurrences fall outside the bounds.

The code under test is ops.ConvLSTMSeq / convlstm_group_forward / convlstm_group_step: Python that strings kernels together.
Every kernel has its own parity suite at the C ABI; this suite takes the tensors the recurrence stored per step
(ops.RECURRENCE_TRACE: h_hist, c_hist, gates, dgates) and checks every step on the device's OWN stored inputs, so the per-step bounds of
those suites apply unchanged:

  forward step t      x_all[t], h_hist[t], c_hist[t] -> gates[t], c_hist[t+1], h_hist[t+1]; the fused-cell bounds of
                      tests/test_gpu_igemm_abi.py with dpre = c * mag, c = f32_coeff(Ktot, ksplit) of the plan that ran.  Hoisted:
                      mag is the sum of the two GEMMs' magnitudes and c the sum of their coefficients (the step that is the
                      point-wise kernel alone has the x GEMM only).
  backward step t     gates[t], c_hist[t], c_hist[t+1], dh_all[t], dgates[t+1] -> dgates[t].  dh_rec = W_h^T (*) dgates[t+1] in f64
                      with E_dh = c * mag (+ half a 16-bit unit x 1.01 on the plan that stores it in 16 bits).  dc is never stored
                      per step: dc_in comes from the reference's own chain and its error is propagated,
                          E_tot(t) = E_dc(t) + |o| (1 - tanh^2 c) E_dh(t),   E_dc(t-1) = |f_t| E_tot(t) + E * mag_dc(t),
                      E_dc(T-1) = 0 (dc_T is an exact input).  dgates[t]: the local bound of test_lstm_bwd_pointwise_against_f64
                      (E * mag, then half a unit x 1.01) plus the first-order sensitivity to the two inexact inputs:
                      |g i(1-i)|, |c_prev f(1-f)|, |i(1-g^2)| times E_tot, |tanh(c) o(1-o)| times E_dh.
  after the loop      dx_all (STORE bound), dW (weight-gradient bound c * (mag + |P|)), db ((2e-6 + blocks * 2^-24) sum|terms|),
                      dh0 (c * mag + half a unit), dc0 (E_dc(-1)), all from the device's dgates.

Weights enter as the 16-bit values the panels hold; the panels are written from the pack descriptors of ops.py through
pack_cases.index_map (pinned to F.conv2d by tests/test_pack_cases_host.py).  All tensors here are NHWC with padded channels, f64,
on the host.
"""
import ctypes as C
from dataclasses import dataclass
from types import SimpleNamespace

import torch

import igemm_cases as IC
import pack_cases as PC
import wgrad_cases as WC
import test_gpu_igemm_abi as IG
import test_gpu_pointwise_abi as PW
import test_gpu_wgrad_abi as WG
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops

F64 = torch.float64
E_ACT = IG.E_ACT                       # one fast_sigmoid / fast_tanh / f32 cell update
E_BWD = PW.LSTM_BWD_E                  # f32 evaluation of the backward point-wise kernel, in units of mag
u16 = IG.u16
tag = IG.tag


def f32_coeff(Ktot, ksplit=1):
    return IG.f32_coeff(SimpleNamespace(Ktot=Ktot), ksplit)


def wgrad_coeff(M, splits):
    return WG.coeff(SimpleNamespace(M=M), splits)


def floor16(dtype):
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


def bound16(ref, f32_term, dtype):
    """Half a 16-bit unit x 1.01 of the reference (fp16: at least half the subnormal spacing) + the f32 term."""
    return (u16(dtype) * 1.01 * ref.abs()).clamp(min=floor16(dtype)) + f32_term + 1e-30


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class RCase:
    name: str
    T: int
    B: int
    H: int
    W: int
    Cx: int
    Hd: int
    k: int = 3
    state: bool = False          # h0 / c0 given and requiring gradients
    dh: str = "all"              # all | none (only c_T is used) | last (zero except at t = T-1)
    dc_T: bool = False
    hoist: bool = False
    force: int = 0               # > 0: split_k_factor patched to return this for the forward pass (a plan the small shape does not reach)
    # the plan the case is meant for: (forward: K ranges of the per-step GEMM, slabs, kernel), (W_h^T: K ranges, slabs, kernel)
    plan: tuple = ()

    @property
    def pixels(self):
        return self.B * self.H * self.W

    @property
    def Hdp(self):
        return ops.cpad(self.Hd)

    @property
    def Cxp(self):
        return ops.cpad(self.Cx)


A = (3, 2, 9, 10, 24, 40)
S = (3, 1, 8, 8, 4, 8)
CASES = [
    RCase("A", *A, plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-state", *A, state=True, dc_T=True, plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-no-dh", *A, dh="none", dc_T=True, plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-state-no-dcT", *A, state=True, plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-dh-last", *A, dh="last", plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-T1", 1, *A[1:], state=True, dc_T=True, plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-T2", 2, *A[1:], plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-T5", 5, *A[1:], state=True, dc_T=True, plan=((2, 2, 0), (3, 3, 1))),
    RCase("S", *S, plan=((2, 2, 1), (1, 1, 1))),
    RCase("S-state", *S, state=True, dc_T=True, plan=((2, 2, 1), (1, 1, 1))),
    RCase("P5", 2, 2, 5, 7, 3, 5, state=True, dc_T=True, plan=((2, 2, 1), (1, 1, 1))),
    RCase("P8", 2, 2, 5, 7, 3, 8, state=True, dc_T=True, plan=((2, 2, 1), (1, 1, 1))),
    RCase("P20", 2, 1, 6, 6, 12, 20, plan=((2, 2, 0), (2, 2, 1))),
    RCase("P40", 2, 1, 6, 6, 12, 40, plan=((2, 2, 0), (3, 3, 1))),
    RCase("A-k1", *A, k=1, state=True, dc_T=True, plan=((1, 0, 0), (1, 1, 1))),
    RCase("A-k5", 2, *A[1:], k=5, state=True, dc_T=True, plan=((6, 2, 0), (9, 3, 0))),
    RCase("A-fused", *A, force=1, state=True, dc_T=True, plan=((1, 0, 0), (3, 3, 1))),
    # hoisted: the h half of A has 9 K-steps (one range, the fused kernel with pre_add); two requested ranges give pre_add beside a slab
    RCase("A-hoist", *A, hoist=True, force=2, plan=((2, 1, 0), (3, 3, 1))),
    RCase("A-hoist-state", *A, hoist=True, force=2, state=True, dc_T=True, plan=((2, 1, 0), (3, 3, 1))),
    RCase("A-hoist-fused", *A, hoist=True, state=True, dc_T=True, plan=((1, 0, 0), (3, 3, 1))),
    RCase("A-hoist-T1", 1, *A[1:], hoist=True, plan=((2, 2, 0), (3, 3, 1))),
    RCase("S-hoist", *S, hoist=True, plan=((1, 0, 0), (1, 1, 1))),
    RCase("S-hoist-state", *S, hoist=True, state=True, dc_T=True, plan=((1, 0, 0), (1, 1, 1))),
]
BY_NAME = {c.name: c for c in CASES}


def plan_of(c: RCase):
    """What ConvLSTMSeq does with this case, from the library's own planners (no GPU): a dict with
    hoist; fwd = (Ktot, ksplit, slabs, kernel) of the per-step GEMM; Ktot_x of the hoisted x GEMM; dh = (Ktot, ksplit, slabs, kernel) of
    the W_h^T launch (slabs = 1 with ksplit = 1: the 16-bit store form)."""
    hoist = c.hoist and c.T >= 2
    pd = ops.lstm_half_pack_desc(c.Hd, c.Cx, "h", c.k) if hoist else ops.lstm_pack_desc(c.Hd, c.Cx, c.k)
    ks = c.force if c.force else ops.split_k_factor(c.pixels, pd.N, pd.Ktot // 64)
    nsl = ops.ksplit_used(pd.Ktot, ks, c.k) if ks > 1 else 0
    srcs = [(c.Hdp, c.H, c.W, 0, 0)] if hoist else [(c.Cxp, c.H, c.W, 0, 0), (c.Hdp, c.H, c.W, 0, 0)]
    ic = IC.Case(c.name, -1, c.B, c.H, c.W, srcs, pd.N, ktap=c.k, pad=c.k // 2, epi=L.EPI_ATOMIC if ks > 1 else L.EPI_LSTM,
                 ksplit=ks, Hd=c.Hd, bias=False)
    assert ic.Ktot == pd.Ktot
    fshape = int(L.lib.uclstm_igemm_fwd_shape(C.byref(IC.dummy_desc(ic))))
    dd = ops.lstm_dgrad_pack_desc(c.Hd, c.Cx, c.Hd, c.k)
    kb = ops.split_k_factor(c.pixels, dd.N, dd.Ktot // 64)
    nb = ops.ksplit_used(dd.Ktot, kb, c.k) if kb > 1 else 1
    bc = IC.Case(c.name, -1, c.B, c.H, c.W, [(4 * c.Hdp, c.H, c.W, 0, 0)], dd.N, ktap=c.k, pad=c.k // 2,
                 epi=L.EPI_ATOMIC if kb > 1 else L.EPI_STORE, ksplit=kb, bias=False)
    assert bc.Ktot == dd.Ktot
    bshape = int(L.lib.uclstm_igemm_fwd_shape(C.byref(IC.dummy_desc(bc))))
    return dict(hoist=hoist, fwd=(pd.Ktot, ks, nsl, fshape), dh=(dd.Ktot, kb, nb, bshape),
                Ktot_x=ops.lstm_half_pack_desc(c.Hd, c.Cx, "x", c.k).Ktot if hoist else 0)


def fwd_coeffs(c: RCase, plan, zero_state: bool):
    """Per step: the coefficient c of dpre = c * mag for the GEMMs that fed the step's pre-activations."""
    Ktot, ks, _, _ = plan["fwd"]
    out = []
    for t in range(c.T):
        if not plan["hoist"]:
            out.append(f32_coeff(Ktot, ks))
        elif t == 0 and zero_state:
            out.append(f32_coeff(plan["Ktot_x"], 1))
        else:
            out.append(f32_coeff(plan["Ktot_x"], 1) + f32_coeff(Ktot, ks))
    return out


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def loss_scale(dtype):
    return PW.loss_scale(dtype)


def pad_last(t, Cp):
    """[..., C] -> [..., Cp] with zero pad channels."""
    out = torch.zeros(t.shape[:-1] + (Cp,), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def make_inputs(c: RCase, dtype, seed=0):
    """NHWC tensors with zero pad channels: x_all / h0 / dh_all in the 16-bit type, c0 / dc_T f32, weight / bias f32 OIHW.
    fp16: gradients x 1024 and at least 0.25 x 1024 in magnitude, weights small enough that every gate stays in
    [0.1, 0.9] (asserted by the tests on the stored gates)."""
    g = torch.Generator().manual_seed(7000 + seed + sum(map(ord, c.name.split("-")[0])) + 13 * c.T + c.k)
    rn = lambda *s: torch.randn(*s, generator=g)
    f16 = dtype == torch.float16
    Sc = loss_scale(dtype)
    fan = c.k * c.k * (c.Cx + c.Hd)
    w = rn(4 * c.Hd, c.Cx + c.Hd, c.k, c.k) * ((0.45 if f16 else 1.6) / fan ** 0.5)
    b = rn(4 * c.Hd) * (0.1 if f16 else 0.3)
    x_all = pad_last(rn(c.T, c.B, c.H, c.W, c.Cx) * 0.8, c.Cxp).to(dtype)

    def grad_like(*s):
        if f16:
            return Sc * PW.signed_away_from_zero(s, 0.25, 2.0)
        return rn(*s)

    torch.manual_seed(int(torch.randint(0, 1 << 30, (1,), generator=g)))
    out = dict(x_all=x_all, weight=w, bias=b, h0=None, c0=None, dh_all=None, dc_T=None)
    if c.state:
        out["h0"] = pad_last(torch.tanh(rn(c.B, c.H, c.W, c.Hd)) * 0.9, c.Hdp).to(dtype)
        out["c0"] = pad_last(rn(c.B, c.H, c.W, c.Hd).clamp(-2.0, 2.0), c.Hdp).float()
    if c.dh != "none":
        dh = pad_last(grad_like(c.T, c.B, c.H, c.W, c.Hd), c.Hdp)
        if c.dh == "last":
            dh[:c.T - 1] = 0
        out["dh_all"] = dh.to(dtype)
    if c.dc_T or c.dh == "none":
        out["dc_T"] = pad_last(grad_like(c.B, c.H, c.W, c.Hd), c.Hdp).float()
    return out


# ---------------------------------------------------------------------------------------------
# f64 references
# ---------------------------------------------------------------------------------------------
class Ref:
    """f64 references of one ConvLSTM layer with gate weight ``w`` [4Hd, Cx+Hd, k, k] (f64: already rounded to the panel type by the
    caller) and bias [4Hd] or None."""

    def __init__(self, w, bias, Hd, Cx, k):
        self.Hd, self.Cx, self.k, self.Hdp, self.Cxp = Hd, Cx, k, ops.cpad(Hd), ops.cpad(Cx)
        w = w.to(F64)
        self.w = w
        self.pd = ops.lstm_pack_desc(Hd, Cx, k)
        self.wp = PC.panel_of(self.pd, w)
        self.wp_x = PC.panel_of(ops.lstm_half_pack_desc(Hd, Cx, "x", k), w)
        self.wp_h = PC.panel_of(ops.lstm_half_pack_desc(Hd, Cx, "h", k), w)
        self.ddh = ops.lstm_dgrad_pack_desc(Hd, Cx, Hd, k)
        self.wd_h = PC.panel_of(self.ddh, w, Cx * k * k)
        self.ddx = ops.lstm_dgrad_pack_desc(Hd, Cx, Cx, k)
        self.wd_x = PC.panel_of(self.ddx, w, 0)
        self.ud = ops.lstm_wgrad_unpack_desc(Hd, Cx, k)
        self.bp = None if bias is None else PC.bias_ref(self.pd, bias.to(F64))

    # -- forward ---------------------------------------------------------------------------
    def fwd_step(self, x_t, h_prev, c_prev):
        """x_t [B,H,W,Cxp], h_prev [B,H,W,Hdp], c_prev [B,H,W,Hdp] or None -> gates [M,4,Hdp], c [M,Hdp], h [M,Hdp], mag [M,4,Hdp]
        (mag = sum_k |A * Wp| of the x and the h GEMM together + |bias|)."""
        B, H, W, _ = x_t.shape
        k = self.k
        pre_x, mag_x = IC.gemm_ref(IC.gather_a(B, H, W, k, 1, k // 2, [(x_t, 0, 0)]), self.wp_x)
        pre_h, mag_h = IC.gemm_ref(IC.gather_a(B, H, W, k, 1, k // 2, [(h_prev, 0, 0)]), self.wp_h)
        pre, mag = pre_x + pre_h, mag_x + mag_h
        if self.bp is not None:
            pre, mag = pre + self.bp, mag + self.bp.abs()
        pre, mag = IC.lstm_rows_to_gates(pre, self.Hdp), IC.lstm_rows_to_gates(mag, self.Hdp)
        cp = torch.zeros(pre.shape[0], self.Hdp, dtype=F64) if c_prev is None else c_prev.to(F64).reshape(-1, self.Hdp)
        gates, cn, hn = IC.lstm_cell_ref(pre, cp)
        return gates, cn, hn, mag

    def fwd_step_two_source(self, x_t, h_prev):
        """The same pre-activations through the two-source panel (what the unhoisted launch multiplies): (pre, mag) [M,4,Hdp]."""
        B, H, W, _ = x_t.shape
        pre, mag = IC.gemm_ref(IC.gather_a(B, H, W, self.k, 1, self.k // 2, [(x_t, 0, 0), (h_prev, 0, 0)]), self.wp)
        if self.bp is not None:
            pre, mag = pre + self.bp, mag + self.bp.abs()
        return IC.lstm_rows_to_gates(pre, self.Hdp), IC.lstm_rows_to_gates(mag, self.Hdp)

    # -- backward --------------------------------------------------------------------------
    def dgrad(self, dg, which="h"):
        """Transposed gate convolution of dg [n,H,W,4Hdp] with W_h (or W_x): (ref, mag) [n*H*W][cpad(channels)]."""
        n, H, W, _ = dg.shape
        Am = IC.gather_a(n, H, W, self.k, 1, self.k // 2, [(dg, 0, 0)])
        return IC.gemm_ref(Am, self.wd_h if which == "h" else self.wd_x)

    @staticmethod
    def bwd_step(gates, c_prev, c_new, dh, dc_in):
        """The header's formulas in f64 on [M,4,Hdp] gates: (dgates [M,4,Hdp], dc' , dc_out)."""
        gi, gf, gg, go = gates[:, 0], gates[:, 1], gates[:, 2], gates[:, 3]
        tc = torch.tanh(c_new)
        dct = dc_in + dh * go * (1 - tc * tc)
        dgt = torch.stack((dct * gg * gi * (1 - gi), dct * c_prev * gf * (1 - gf), dct * gi * (1 - gg * gg), dh * tc * go * (1 - go)), 1)
        return dgt, dct, dct * gf

    def wgrad(self, x_all, hprev_all, dgates, base=None):
        """dW [4Hd, Cx+Hd, k, k] = unpack(gather_dy^T @ gather_a) over x_all [T,B,H,W,Cxp] and hprev_all [T,B,H,W,Hdp]: (ref, mag, mapped)
        flat over the weight; ``base``: a gradient the result is accumulated onto."""
        T, B, H, W, _ = x_all.shape
        n = T * B
        dg = dgates.reshape(n, H, W, 4 * self.Hdp)
        ref, mag = WC.wgrad_ref(n, H, W, self.ud.N, self.k, 1, self.k // 2,
                                [(x_all.reshape(n, H, W, -1), 0, 0), (hprev_all.reshape(n, H, W, -1), 0, 0)],
                                [(dg, 0, 4 * self.Hdp, 0, 1, 0, 0)])
        # |slab| enters unpack_ref's mag: put the magnitudes through the same map
        b0 = torch.zeros(self.w.numel(), dtype=F64) if base is None else base.to(F64).reshape(-1)
        r, _, mapped = PC.unpack_ref(self.ud, ref[None], b0, base is not None)
        m, _, _ = PC.unpack_ref(self.ud, mag[None], b0.abs(), base is not None)
        return torch.from_numpy(r), torch.from_numpy(m), torch.from_numpy(mapped)

    def bgrad(self, dgates):
        """db [4Hd] = column sums of the valid columns of dgates [..., 4Hdp]: (ref, sum|terms|)."""
        d = dgates.to(F64).reshape(-1, 4, self.Hdp)[:, :, :self.Hd]
        return d.sum(0).reshape(-1), d.abs().sum(0).reshape(-1)


# ---------------------------------------------------------------------------------------------
# step-by-step comparison
# ---------------------------------------------------------------------------------------------
def _ratio(err, bound):
    return float((err / bound).max()) if err.numel() else 0.0


def check_forward(c, dtype, ref: Ref, coeffs, x_all, h_hist, c_hist, gates, zero_c0):
    """Every step of the stored forward history against the f64 cell on the step's stored inputs.  ``coeffs``: fwd_coeffs().
    Returns {output: worst |err| / bound}; nothing is asserted here but the exact zeros of the pad channels."""
    T, Hd, Hdp = x_all.shape[0], ref.Hd, ref.Hdp
    worst = {"c": 0.0, "h": 0.0, "gates": 0.0}
    for t in range(T):
        c_prev = None if (zero_c0 and t == 0) else c_hist[t]
        gref, cref, href, mag = ref.fwd_step(x_all[t].double(), h_hist[t].double(), c_prev)
        dpre = coeffs[t] * mag
        dg = torch.stack((dpre[:, 0] / 4, dpre[:, 1] / 4, dpre[:, 2], dpre[:, 3] / 4), 1) + E_ACT
        cp = torch.zeros_like(cref) if c_prev is None else c_prev.double().reshape(-1, Hdp)
        dc = cp.abs() * dg[:, 1] + gref[:, 2].abs() * dg[:, 0] + gref[:, 0].abs() * dg[:, 2] + E_ACT
        cgot = c_hist[t + 1].double().reshape(-1, Hdp)
        hgot = h_hist[t + 1].double().reshape(-1, Hdp)
        worst["c"] = max(worst["c"], _ratio((cgot - cref).abs(), dc + 1e-30))
        worst["h"] = max(worst["h"], _ratio((hgot - href).abs(), bound16(href, dg[:, 3] + dc + E_ACT, dtype)))
        if gates is not None:
            ggot = gates[t].double().reshape(-1, 4, Hdp)
            worst["gates"] = max(worst["gates"], _ratio((ggot - gref).abs(), bound16(gref, dg, dtype)))
        assert bool((cgot[:, Hd:] == 0).all()) and bool((hgot[:, Hd:] == 0).all()), f"{c.name} t={t}: pad hidden channels of h / c not 0"
    return worst


def check_backward(c, dtype, ref: Ref, plan, *, x_all, h_hist, c_hist, gates, dgates, dh_all, dc_T, has_c0, out, wgrad_splits=1,
                   base_w=None, base_b=None, colsum_blocks=None):
    """Every step of the stored dgates against the f64 point-wise formulas, then the outputs in ``out`` (dx, dh0, dc0, dW, db; None =
    not produced) against their references on the device's dgates.  Returns {output: worst |err| / bound}."""
    T, B, H, W, _ = x_all.shape
    Hd, Hdp, M = ref.Hd, ref.Hdp, B * H * W
    Ktot_b, ks_b, nsl_b, _ = plan["dh"]
    store16 = ks_b == 1
    cdh = f32_coeff(Ktot_b, ks_b)
    zeros = torch.zeros(M, Hdp, dtype=F64)
    dc_ref = zeros if dc_T is None else dc_T.double().reshape(M, Hdp)
    E_dc = zeros
    worst = {"dgates": 0.0}
    dgd = dgates.double()
    assert bool((dgd.reshape(T, M, 4, Hdp)[..., Hd:] == 0).all()), f"{c.name}: pad channels of dgates not 0"

    def rec_of(dg_next):
        r, m = ref.dgrad(dg_next, "h")
        e = cdh * m
        if store16:
            e = e + (u16(dtype) * 1.01 * r.abs()).clamp(min=floor16(dtype))
        return r, m, e

    for t in range(T - 1, -1, -1):
        g = gates[t].double().reshape(M, 4, Hdp)
        gi, gf, gg, go = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
        cp = c_hist[t].double().reshape(M, Hdp) if (has_c0 or t > 0) else zeros
        cn = c_hist[t + 1].double().reshape(M, Hdp)
        dha = zeros if dh_all is None else dh_all[t].double().reshape(M, Hdp)
        rec, recmag, E_dh = (zeros, zeros, zeros) if t == T - 1 else rec_of(dgd[t + 1])
        dh, dhmag = dha + rec, dha.abs() + recmag + E_dh
        dref, dct, dc_out = Ref.bwd_step(g, cp, cn, dh, dc_ref)
        tc = torch.tanh(cn)
        mct = dc_ref.abs() + E_dc + dhmag * go
        mag = torch.stack((mct * gg.abs() * gi * (1 - gi), mct * cp.abs() * gf * (1 - gf), mct * gi * (1 + gg * gg), dhmag * go * (1 - go)), 1)
        E_tot = E_dc + go * (1 - tc * tc) * E_dh
        sens = torch.stack(((gg * gi * (1 - gi)).abs() * E_tot, (cp * gf * (1 - gf)).abs() * E_tot, (gi * (1 - gg * gg)).abs() * E_tot,
                            (tc * go * (1 - go)).abs() * E_dh), 1)
        got = dgd[t].reshape(M, 4, Hdp)
        worst["dgates"] = max(worst["dgates"], _ratio((got - dref).abs(), bound16(dref, E_BWD * mag + sens, dtype)))
        dc_ref, E_dc = dc_out, gf.abs() * E_tot + E_BWD * mct * gf
    if out.get("dc0") is not None:
        got = out["dc0"].double().reshape(M, Hdp)
        worst["dc0"] = _ratio((got - dc_ref).abs(), E_dc + 1e-30)
        assert bool((got[:, Hd:] == 0).all()), f"{c.name}: pad channels of dc0 not 0"
    if out.get("dh0") is not None:
        r, m, _ = rec_of(dgd[0])
        got = out["dh0"].double().reshape(M, Hdp)
        worst["dh0"] = _ratio((got - r).abs(), bound16(r, cdh * m, dtype))
        assert bool((got[:, Hd:] == 0).all()), f"{c.name}: pad channels of dh0 not 0"
    if out.get("dx") is not None:
        r, m = ref.dgrad(dgd.reshape(T * B, H, W, 4 * Hdp), "x")
        got = out["dx"].double().reshape(T * M, -1)
        worst["dx"] = _ratio((got - r).abs(), bound16(r, 2.0 ** -21 * m, dtype))
        assert bool((got[:, ref.Cx:] == 0).all()), f"{c.name}: pad channels of dx not 0"
    if out.get("dW") is not None:
        r, m, mapped = ref.wgrad(x_all.double(), h_hist[:T].double(), dgd, base_w)
        assert bool(mapped.all())
        got = out["dW"].double().reshape(-1)
        worst["dW"] = _ratio((got - r).abs(), wgrad_coeff(T * M, wgrad_splits) * m + 1e-30)
    if out.get("db") is not None:
        r, terms = ref.bgrad(dgd)
        blocks = colsum_blocks if colsum_blocks is not None else int(L.lib.uclstm_colsum_ordered_rows(T * M, 4 * Hdp))
        if base_b is not None:
            r, terms = r + base_b.double(), terms + base_b.double().abs()
        got = out["db"].double().reshape(-1)
        worst["db"] = _ratio((got - r).abs(), (2e-6 + blocks * 2.0 ** -24) * terms + 1e-30)
    return worst
