"""Host-side restatements for the vector-target path (VectorNPZDataset, uclstm_dataset_gather_vec, uclstm_plane_d4_vec,
uclstm_metric_sums_vec), shared by tests/test_vector_host.py and the GPU tests.

Three independent statements of what a move does to a vector field:
  * ``generator_map``: the rules of the issue composed from the three generators (h, then v, then t);
  * ``apply_map``: a channel map applied to moved planes with torch alone (flip / transpose / index / negate);
  * ``potential_field``: the PHYSICS, with no reference to any channel rule.  phi(i, j) is a polynomial with integer coefficients;
    a move relabels the pixels, phi'(i', j') = phi(a(i', j'), b(i', j')) with the index formula of the codes, and the gradient of
    phi' follows from the chain rule alone.  A dataset channel "+w" holds d phi / d j (along columns), "+h" holds d phi / d i (along
    rows), "-w" / "-h" their negatives, None holds phi itself.  Every value is an integer below 2^24: exact in f32.
"""
import numpy as np
import torch

AXES_UVW = ("+w", "-h", None)                       # u east, v north on rows that run south, w a scalar


def torch_move(s, code):
    if code & 1:
        s = s.flip(-1)
    if code & 2:
        s = s.flip(-2)
    if code & 4:
        s = s.transpose(-2, -1)
    return s


def inv(c):
    return c if not c & 4 else 4 | (c & 1) << 1 | (c & 2) >> 1


def _sign(a):
    return 1 if a[0] == "+" else -1


def generator_map(axes, code):
    """[(source channel, negate)] per output channel: h, v, t applied one after the other, each as the issue words it."""
    w = [c for c, a in enumerate(axes) if a is not None and a[1] == "w"]
    h = [c for c, a in enumerate(axes) if a is not None and a[1] == "h"]
    ident = [(c, False) for c in range(len(axes))]

    def compose(first, then):
        return [(first[src][0], first[src][1] != neg) for src, neg in then]

    cur = list(ident)
    if code & 1:
        g = list(ident)
        for c in w:
            g[c] = (c, True)
        cur = compose(cur, g)
    if code & 2:
        g = list(ident)
        for c in h:
            g[c] = (c, True)
        cur = compose(cur, g)
    if code & 4:
        g = list(ident)
        if w and h:
            neg = _sign(axes[w[0]]) * _sign(axes[h[0]]) < 0
            g[w[0]], g[h[0]] = (h[0], neg), (w[0], neg)
        elif w or h:
            raise ValueError("unpaired horizontal channel")
        cur = compose(cur, g)
    return cur


def apply_map(t, code, cmap):
    """``t [..., Cy, H, W]`` moved by ``code``, channels taken and negated as ``cmap`` says -- torch only."""
    moved = torch_move(t, code)
    return torch.stack([-moved[..., src, :, :] if neg else moved[..., src, :, :] for src, neg in cmap], dim=-3)


# phi = 2 i^3 - 3 i^2 j + 5 i j^2 - j^3 + 4 i^2 - 7 i j + 6 j^2 + 11 i - 13 j + 17
def _phi(i, j):
    return 2 * i ** 3 - 3 * i ** 2 * j + 5 * i * j ** 2 - j ** 3 + 4 * i ** 2 - 7 * i * j + 6 * j ** 2 + 11 * i - 13 * j + 17


def _phi_i(i, j):
    return 6 * i ** 2 - 6 * i * j + 5 * j ** 2 + 8 * i - 7 * j + 11


def _phi_j(i, j):
    return -3 * i ** 2 + 10 * i * j - 3 * j ** 2 - 7 * i + 12 * j - 13


def potential_field(axes, S, code=0):
    """The dataset channels ``[Cy, S, S]`` (int64) of the potential phi MOVED by ``code`` on an S x S frame: the moved potential is
    phi'(i', j') = phi(a, b), (a, b) = (j', i') with t else (i', j'), then a = S-1-a with v, b = S-1-b with h; its gradient by
    the chain rule."""
    ii, jj = np.meshgrid(np.arange(S, dtype=np.int64), np.arange(S, dtype=np.int64), indexing="ij")
    # (a, b) as affine functions of (i', j'): a = a0 + a_i i' + a_j j'
    a_i, a_j, b_i, b_j = (0, 1, 1, 0) if code & 4 else (1, 0, 0, 1)
    a0 = b0 = 0
    if code & 2:
        a0, a_i, a_j = S - 1, -a_i, -a_j
    if code & 1:
        b0, b_i, b_j = S - 1, -b_i, -b_j
    a, b = a0 + a_i * ii + a_j * jj, b0 + b_i * ii + b_j * jj
    d_i = _phi_i(a, b) * a_i + _phi_j(a, b) * b_i              # d phi' / d i'
    d_j = _phi_i(a, b) * a_j + _phi_j(a, b) * b_j              # d phi' / d j'
    planes = []
    for ax in axes:
        if ax is None:
            planes.append(_phi(a, b))
        else:
            planes.append(_sign(ax) * (d_j if ax[1] == "w" else d_i))
    out = np.stack(planes)
    assert np.abs(out).max() < 2 ** 24
    return out


def normalise64(raw, ds, clip=False):
    """``VectorNPZDataset.__getitem__`` on raw ``[..., Cy, H, W]`` in f64 (clipping off unless asked)."""
    raw = np.asarray(raw, dtype=np.float64)
    out = np.empty_like(raw)
    for c in range(raw.shape[-3]):
        v = raw[..., c, :, :]
        if clip:
            v = np.clip(v, ds.min_vel[c], ds.max_vel[c])
        if ds.y_transform == "asinh":
            v = np.arcsinh(v / ds.y_scale[c])
        elif ds.y_transform == "signed_log":
            v = np.sign(v) * np.log1p(np.abs(v) / ds.y_scale[c])
        out[..., c, :, :] = 2 * (v - ds.trans_min[c]) / (ds.trans_max[c] - ds.trans_min[c]) - 1.0
    return out


def apply_affine(t, code, affine):
    """``t [..., Cy, H, W]`` (torch) through ``tta_affine``'s triples, in t's dtype."""
    moved = torch_move(t, code)
    return torch.stack([sign * moved[..., src, :, :] + off for src, sign, off in affine], dim=-3)


def denorm64(v, ds, c):
    """Channel ``c`` de-normalised in f64 (torch)."""
    yt = (v.double() + 1.0) / 2.0 * (float(ds.trans_max[c]) - float(ds.trans_min[c])) + float(ds.trans_min[c])
    if ds.y_transform == "asinh":
        return torch.sinh(yt) * float(ds.y_scale[c])
    if ds.y_transform == "signed_log":
        return torch.sign(yt) * torch.expm1(yt.abs()) * float(ds.y_scale[c])
    return yt


def metric_sums64(yp, y, mask, ds):
    """f64 ``[Cy, 4]`` of uclstm_metric_sums_vec: sum |d| m, sum d^2 m, sum d m, sum m per channel; mask ``[..., 1, H, W]`` or None.
    De-normalised in f32 steps as the kernel's inputs are f32, the difference and the sums in f64."""
    Cy = y.shape[-3]
    m = torch.ones_like(y[..., :1, :, :]).double() if mask is None else (mask != 0).double()
    rows = []
    for c in range(Cy):
        d = denorm64(yp[..., c:c + 1, :, :], ds, c) - denorm64(y[..., c:c + 1, :, :], ds, c)
        rows.append(torch.stack(((d.abs() * m).sum(), (d * d * m).sum(), (d * m).sum(), m.sum())))
    return torch.stack(rows)


def write_npz(path, N, T, C, Cy, H, W, seed, scales=(9.0, 9.0, 2.0, 5.0)):
    """A raw vector dataset: X as tests/test_gpu_augment.py draws it, Y channel c ~ scales[c] * N(0, 1) (u, v reach further than w),
    with the values at which the arithmetic can go wrong planted: raw channel 0 around float32(1.1), targets outside the clip
    range, signed zeros."""
    rng = np.random.default_rng(seed)
    X = (rng.random((N, T, C, H, W)) * 40).astype(np.float32)
    X[X < 8] = 0.0
    Y = np.stack([(rng.standard_normal((N, T, H, W)) * scales[c]).astype(np.float32) for c in range(Cy)], axis=2)
    t = np.float32(1.1)
    X[0, 0, 0].reshape(-1)[:3] = [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(2))]
    X[-1, -1, 0].reshape(-1)[-3:] = X[0, 0, 0].reshape(-1)[:3]
    for c in range(Cy):
        Y[0, 0, c].reshape(-1)[:5] = [-60.0, 45.0, 0.0, -0.0, 1e-30]
        Y[-1, -1, c].reshape(-1)[-3:] = [0.0, 70.0, -0.0]
    np.savez(path, X=X, Y=Y)
    return X, Y
