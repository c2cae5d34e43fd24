"""SyncBatchNorm at the C ABI: uclstm_bn_stats_partial / uclstm_bn_stats_from_sums and uclstm_bn_bwd_sums_stage / _finish.

Shapes, data recipe and RTOL are those of tests/test_gpu_pointwise_abi.py::test_bn_statistics_against_f64 (copied, that file is
not imported): data with |mean| / std up to 30, so that var = E2 - m^2 cancels three digits.
  (i)   the f64 sums against numpy: |error| <= tpg * 2^-53 * sum |terms| (worst case of f64 recursive summation of tpg terms);
  (ii)  one rank: partial -> from_sums is bit-identical to uclstm_bn_stats_fwd (scale, shift, mean, rstd, tile-0 slots, pads);
  (iii) two simulated ranks: two partial tensors, f64 sums added on the host, from_sums with the doubled count against the f64
        formulas within RTOL (shift relative to |beta| + |mean*scale|);
  (iv)  stage -> finish: inv_world = 1 returns the bits of `sums`; two buffers added and inv_world = 0.5 give
        float((a64 + b64) / 2) exactly.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

DEV = "cuda"
# (groups, tiles per group, Cp, C)
BN_STATS_SHAPES = [
    (3, 1, 8, 5),                 # one tile per group; C < Cp
    (2, 17, 72, 67),              # tiles % 16 != 0; partly filled second 64-channel slab; C < Cp
    (5, 40, 200, 200),            # several groups, C = Cp
]
RTOL = 2.0 ** -21
PER_TILE, EPS = 24, 1e-5


def make_partials(shape, seed_offset=0):
    """The recipe of test_bn_statistics_against_f64: f32 per-tile (sum, sum of squares) [groups][tpg][Cp][2], gamma, beta."""
    groups, tpg, Cp, C = shape
    torch.manual_seed(500 + tpg + Cp + seed_offset)
    std = torch.rand(Cp) + 0.5
    ratio = (torch.rand(Cp) * 29 + 1) * (torch.randint(0, 2, (Cp,)).float() * 2 - 1)
    x = (ratio * std)[None, None, None, :] * (1 + 0.05 * torch.randn(groups, 1, 1, Cp)) + std * torch.randn(groups, tpg, PER_TILE, Cp)
    x[..., C:] = 0.0
    stats = torch.stack((x.double().sum(2), (x.double() ** 2).sum(2)), -1).float()
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    gamma[::4] *= -1.0
    return stats, gamma, beta


def dev(t):
    return t.contiguous().to(DEV)


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def partial(st, shape):
    groups, tpg, Cp, _ = shape
    s64 = nan_like((groups, Cp, 2), torch.float64)
    U._lib.check(U._lib.lib.uclstm_bn_stats_partial(ops._p(st), groups, tpg, Cp, ops._p(s64), ops._stream()), "bn_stats_partial")
    return s64


def from_sums(s64, count, st, shape, gd, bd):
    groups, tpg, Cp, C = shape
    outs = [nan_like((groups, Cp), torch.float32) for _ in range(4)]
    U._lib.check(U._lib.lib.uclstm_bn_stats_from_sums(ops._p(s64), count, ops._p(st), groups, tpg, Cp, C, ops._p(gd), ops._p(bd), EPS,
                                                      *[ops._p(t) for t in outs], ops._stream()), "bn_stats_from_sums")
    return outs


def check_rtol(got, ref, what, rtol=RTOL, scale=None):
    got = got.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    e = float(((got - ref).abs() / ((ref.abs() if scale is None else scale) + 1e-300)).max())
    print(f"[parity] {what}: max relative error {e:.2e} (<= {rtol:.2e})")
    assert e <= rtol, f"{what}: {e:.3e} > {rtol:.3e}"


@pytest.mark.parametrize("shape", BN_STATS_SHAPES, ids=str)
def test_partial_sums_against_numpy_f64(shape):
    groups, tpg, Cp, C = shape
    stats, _, _ = make_partials(shape)
    st = dev(stats)
    s64 = partial(st, shape)
    torch.cuda.synchronize()
    assert torch.equal(st.cpu(), stats), "bn_stats_partial must not consume `stats`"
    a = stats.numpy().astype(np.float64)
    want, mag = a.sum(axis=1), np.abs(a).sum(axis=1)
    got = s64.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want)
    bound = tpg * 2.0 ** -53 * mag
    worst = float((err / np.maximum(mag, 1e-300)).max())
    print(f"[parity] bn_stats_partial {shape}: max |error| / sum|terms| {worst:.2e} (<= {tpg * 2.0 ** -53:.2e})")
    assert (err <= bound).all()
    assert (got[:, C:] == 0).all()


@pytest.mark.parametrize("shape", BN_STATS_SHAPES, ids=str)
def test_one_rank_is_bit_identical_to_bn_stats_fwd(shape):
    groups, tpg, Cp, C = shape
    stats, gamma, beta = make_partials(shape)
    count = tpg * PER_TILE
    gd, bd = dev(gamma), dev(beta)
    st_ref = dev(stats)
    ref = [nan_like((groups, Cp), torch.float32) for _ in range(4)]
    U._lib.check(U._lib.lib.uclstm_bn_stats_fwd(ops._p(st_ref), groups, tpg, Cp, C, count, ops._p(gd), ops._p(bd), EPS,
                                                *[ops._p(t) for t in ref], ops._stream()), "bn_stats_fwd")
    st = dev(stats)
    outs = from_sums(partial(st, shape), count, st, shape, gd, bd)
    torch.cuda.synchronize()
    for k, a, b in zip(("scale", "shift", "mean", "rstd"), outs, ref):
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{k}: not the bits of bn_stats_fwd"
        assert bool((a[:, C:] == 0).all()), f"{k}: pad channels not zero"
    assert torch.equal(st.view(torch.int32), st_ref.view(torch.int32)), "stats (tile-0 slots, everything else untouched) differ"
    # ... and the running statistics that follow from the tile-0 slots are then the same too
    print(f"[parity] bn_stats_partial -> bn_stats_from_sums {shape}: scale, shift, mean, rstd, stats bit-identical to bn_stats_fwd")


@pytest.mark.parametrize("shape", BN_STATS_SHAPES, ids=str)
def test_two_simulated_ranks_against_f64(shape):
    groups, tpg, Cp, C = shape
    stats_a, gamma, beta = make_partials(shape)
    stats_b, _, _ = make_partials(shape, seed_offset=1000)
    count = 2 * tpg * PER_TILE
    gd, bd = dev(gamma), dev(beta)
    st_a, st_b = dev(stats_a), dev(stats_b)
    s64 = dev(partial(st_a, shape).cpu() + partial(st_b, shape).cpu())          # the all-reduce, on the host
    outs = from_sums(s64, count, st_a, shape, gd, bd)
    torch.cuda.synchronize()
    t64 = stats_a.double().sum(1) + stats_b.double().sum(1)
    m = t64[..., 0] / count
    var = (t64[..., 1] / count - m * m).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    live = (torch.arange(Cp) < C).double()
    g64, b64 = torch.zeros(Cp, dtype=torch.float64), torch.zeros(Cp, dtype=torch.float64)
    g64[:C], b64[:C] = gamma.double(), beta.double()
    want = dict(mean=m * live, rstd=rstd * live, scale=g64 * rstd * live, shift=(b64 - m * g64 * rstd) * live)
    shift_scale = b64.abs() + (m * g64 * rstd).abs()
    for k, t in zip(("scale", "shift", "mean", "rstd"), outs):
        got = t.cpu()
        assert bool((got[:, C:] == 0).all()), f"{k}: pad channels not zero"
        if k == "shift":
            check_rtol(got[:, :C], want[k][:, :C], f"syncbn 2 ranks shift {shape}", scale=shift_scale[:, :C])
        else:
            check_rtol(got[:, :C], want[k][:, :C], f"syncbn 2 ranks {k} {shape}")
    slot = st_a.cpu()[:, 0, :C]
    check_rtol(slot[..., 0], m[:, :C], f"syncbn 2 ranks tile-0 mean {shape}")
    check_rtol(slot[..., 1], var[:, :C], f"syncbn 2 ranks tile-0 variance {shape}")
    if tpg > 1:
        assert torch.equal(st_a.cpu()[:, 1:], stats_a[:, 1:]), "from_sums wrote outside the tile-0 slots"


@pytest.mark.parametrize("shape", BN_STATS_SHAPES, ids=str)
def test_backward_sums_stage_and_finish(shape):
    groups, _, Cp, _ = shape
    lib = U._lib.lib
    torch.manual_seed(900 + Cp)
    a = torch.randn(groups, Cp, 2) * torch.logspace(-20, 20, Cp)[None, :, None]
    b = torch.randn(groups, Cp, 2) * torch.logspace(-20, 20, Cp)[None, :, None]
    a[0, 0, 0], a[0, 0, 1] = 0.0, -0.0
    n = a.numel()
    ad, bd = dev(a), dev(b)

    def stage(t):
        s64 = nan_like(tuple(t.shape), torch.float64)
        U._lib.check(lib.uclstm_bn_bwd_sums_stage(ops._p(t), ops._p(s64), n, ops._stream()), "bn_bwd_sums_stage")
        return s64

    def finish(s64, inv_world):
        out = nan_like(tuple(s64.shape), torch.float32)
        U._lib.check(lib.uclstm_bn_bwd_sums_finish(ops._p(s64), inv_world, ops._p(out), n, ops._stream()), "bn_bwd_sums_finish")
        return out

    a64, b64 = stage(ad), stage(bd)
    one = finish(a64, 1.0)
    two = finish(dev(a64.cpu() + b64.cpu()), 0.5)
    torch.cuda.synchronize()
    assert torch.equal(ad.cpu(), a), "bn_bwd_sums_stage must leave `sums` untouched"
    assert torch.equal(a64.cpu(), a.double())
    assert torch.equal(one.cpu().view(torch.int32), a.view(torch.int32)), "stage -> finish(1.0) is not the identity on the bits"
    want = ((a.double() + b.double()) / 2).float()
    assert torch.equal(two.cpu().view(torch.int32), want.view(torch.int32)), "finish(0.5) != float((a64 + b64) / 2)"
