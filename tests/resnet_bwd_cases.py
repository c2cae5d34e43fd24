"""f64 references of the encoder's backward pass (csrc/resnet_bwd.hip and the strided descriptors of resnet.py), each one checked
against torch's own autograd in f64 by tests/test_resnet_bwd_host.py.  Inputs are the 16-bit values the device holds, NHWC."""
import torch
import torch.nn.functional as F

from resnet_cases import nchw, nhwc


# ---------------------------------------------------------------------------------------------
# MaxPool2d(3, 2, 1) backward
# ---------------------------------------------------------------------------------------------
def maxpool3s2_bwd_ref(a, dp, dskip=None):
    """(da, sum of the magnitudes of its terms): dp goes to the FIRST maximum of every clipped window in scan order, the windows'
    contributions and dskip are summed.  a [n,H,W,C], dp [n,Ho,Wo,C]."""
    a, dp = nchw(a.double()), nchw(dp.double())
    n, Cc, H, W = a.shape
    ap = F.pad(a, (1, 1, 1, 1), value=float("-inf"))
    cols = F.unfold(ap, 3, stride=2).view(n, Cc, 9, -1)                        # [n, C, tap in scan order, Ho*Wo]
    assert cols.shape[3] == dp.shape[2] * dp.shape[3]
    is_max = cols == cols.max(2, keepdim=True).values
    first = is_max & (is_max.cumsum(2) == 1)
    g = torch.where(first, dp.reshape(n, Cc, 1, -1).expand_as(cols), torch.zeros_like(cols))
    fold = lambda t: F.fold(t.reshape(n, Cc * 9, -1), (H + 2, W + 2), 3, stride=2)[:, :, 1:-1, 1:-1]
    da, mag = fold(g), fold(g.abs())
    if dskip is not None:
        da, mag = da + nchw(dskip.double()), mag + nchw(dskip.double()).abs()
    return nhwc(da), nhwc(mag)


def relu_with_ties(shape, dtype, seed):
    """A post-ReLU activation with exact ties everywhere: two thirds exact zeros, the rest small integers (exact in bf16 and
    fp16), so that most windows hold their maximum more than once -- at zero or at a positive value."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).clamp(min=0.0).round().to(dtype)


# ---------------------------------------------------------------------------------------------
# relu(bn(z) + bn_r(r)) backward
# ---------------------------------------------------------------------------------------------
def tail_preactivation(z, scale, shift, r, rscale, rshift):
    u = z.double() * scale.double() + shift.double()
    return u + (r.double() if rscale is None else r.double() * rscale.double() + rshift.double())


def tail_sums_ref(u, x, mean, rstd, da):
    """g = da*[u > 0], xhat, sums [Cp][2] = (sum g, sum g*xhat) and the sums of the magnitudes, over the pixels (dim 0)."""
    g = torch.where(u > 0, da.double(), torch.zeros_like(u))
    xhat = (x.double() - mean.double()) * rstd.double()
    return g, xhat, torch.stack((g.sum(0), (g * xhat).sum(0)), -1), torch.stack((g.abs().sum(0), (g * xhat).abs().sum(0)), -1)


def tail_dx_ref(g, xhat, x, scale, mean, rstd, sums):
    """scale*(g - s1/n - xhat*s2/n) with the sums the apply kernel was given, and the magnitude of the regrouped form the kernels
    evaluate, scale*g + k1*x + k0 (tests/test_gpu_pointwise_abi.py: dz_reference)."""
    n = g.shape[0]
    s1, s2, sc = sums[:, 0].double(), sums[:, 1].double(), scale.double()
    ref = sc * (g - s1 / n - xhat * s2 / n)
    k1 = (sc * rstd.double()).abs() * s2.abs() / n
    mag = sc.abs() * (g.abs() + s1.abs() / n) + k1 * (x.double().abs() + mean.double().abs())
    return ref, mag


# ---------------------------------------------------------------------------------------------
# input gradient of conv3x3 / stride 2 / pad 1 (+ conv1x1 / stride 2) as four stride-1 problems
# ---------------------------------------------------------------------------------------------
def s2_dgrad_ref(dz, w, dz_ds=None, w_ds=None):
    """dx [n, 2Ho, 2Wo, Ci] in f64 from the rearranged weight: parity (py, px) of the input pixel reads dz at (j + ty, i + tx),
    ty, tx in {0, 1} (zero beyond the grid), through resnet.s2_dgrad_weight.  dz [n,Ho,Wo,Co] NHWC, w [Co,Ci,3,3]."""
    from unet_convlstm_amd import resnet as R
    wr = R.s2_dgrad_weight(w, w_ds).double()          # [Co (+ Co), Ci, 2, 2, 2, 2]
    src = dz.double() if dz_ds is None else torch.cat([dz.double(), dz_ds.double()], -1)
    n, Ho, Wo, _ = src.shape
    sp = F.pad(src, (0, 0, 0, 1, 0, 1))                                         # one zero row / column beyond the grid
    dx = src.new_zeros(n, 2 * Ho, 2 * Wo, w.shape[1])
    for py in (0, 1):
        for px in (0, 1):
            acc = 0
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = acc + torch.einsum("nhwo,oc->nhwc", sp[:, ty:ty + Ho, tx:tx + Wo], wr[:, :, py, px, ty, tx])
            dx[:, py::2, px::2] = acc
    return dx
