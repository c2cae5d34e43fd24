"""Training / evaluation step loop of the reference's main.py on the HIP path, plus data sources.

``train_one_epoch`` / ``evaluate`` keep the reference signatures and return values
(main.py:77-144, :150-205: ``(avg_loss, mae, rmse, mean_err)`` in de-normalised units) but keep
the metric block on the device as running sums instead of per-pixel Python lists
(main.py:114-133), and do not synchronise with the host inside the step.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import ops
from .loss import compute_loss, check_spec, LossSpec
from .optim import FusedAdamW, WeightEMA


# ---------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------
class SyntheticSequences:
    """Seeded synthetic batches in the post-normalisation ranges of the reference dataset
    (X ~ U[0,1) as after ``x / norm_const``, train/unet.py:283; Y ~ U(-1,1) as
    after the [-1,1] mapping, ``:299``; mask = cloud pixels).  ``kind='blobs'`` draws moving blobs with
    integer velocities in [-5,5] and the bounce rule of digits/build_moving_mnist.py:38-47; X is the frame
    duplicated into both "satellite" channels and Y the per-pixel vx map."""

    def __init__(self, B: int, T: int, H: int, W: int, seed: int = 1, kind: str = "uniform", device="cuda", channels: int = 2):
        g = torch.Generator(device="cpu").manual_seed(seed)
        if kind == "uniform":
            x = torch.rand((B, T, channels, H, W), generator=g)
            y = torch.rand((B, T, 1, H, W), generator=g) * 2 - 1
            mask = (torch.rand((B, T, 1, H, W), generator=g) > 0.3).float()
        elif kind == "blobs":
            x = torch.zeros((B, T, channels, H, W))
            y = torch.zeros((B, T, 1, H, W))
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            for b in range(B):
                for _ in range(2):
                    r = 4 + int(torch.randint(0, 4, (1,), generator=g))
                    px = float(torch.randint(r, W - r, (1,), generator=g))
                    py = float(torch.randint(r, H - r, (1,), generator=g))
                    vx = int(torch.randint(-5, 6, (1,), generator=g))
                    vy = int(torch.randint(-5, 6, (1,), generator=g))
                    for t in range(T):
                        # bump 1/(1+q)^2 in f64 from IEEE basic operations only (+, *, /): bit-identical on every host CPU
                        # (exp() differs by an ulp between vector ISAs, which breaks seed-regenerated fixtures)
                        q = ((xx - px).double() ** 2 + (yy - py).double() ** 2) / (2.0 * (r / 2.0) ** 2)
                        blob = (1.0 / ((1.0 + q) * (1.0 + q))).float()
                        on = blob > 0.1
                        x[b, t, :, on] = torch.maximum(x[b, t, :, on], blob[on])
                        y[b, t, 0][on] = vx / 5.0
                        px, py = px + vx, py + vy
                        if px < r or px > W - 1 - r:
                            vx = -vx
                            px = min(max(px, r), W - 1 - r)
                        if py < r or py > H - 1 - r:
                            vy = -vy
                            py = min(max(py, r), H - 1 - r)
            mask = (x[:, :, 0:1] > 0.1).float()
        else:
            raise ValueError(kind)
        self.x, self.y, self.mask = x.to(device), y.to(device), mask.to(device)

    def __iter__(self):
        yield self.x, self.y, self.mask

    def __len__(self):
        return 1


class NPZSequenceDataset(torch.utils.data.Dataset):
    """Host-side mirror of the reference dataset (train/unet.py:210-327): ``.npz`` with ``X [N,T,2,H,W]``,
    ``Y [N,T,1,H,W]``; mask from RAW x > 1.1 (``:279``), x / max(x_max, 1) (``:220,:283``), Y clipped, asinh(y/scale)
    and mapped to [-1,1] (``:287-299``).  ``denormalize`` accepts numpy or torch (any device) and stays on the
    input's device for tensors."""

    def __init__(self, npz_path, lower_percentile=0.00001, upper_percentile=99.99999, clip_outliers=True,
                 min_y=-7.5987958908081055, max_y=8.784920692443848, y_transform="asinh", y_transform_scale=None,
                 y_transform_percentile=99):
        with np.load(npz_path, allow_pickle=False) as data:
            self.X = data["X"].astype(np.float32)
            self.Y = data["Y"].astype(np.float32)
        self.N, self.T, _, self.H, self.W = self.X.shape
        self.x_max = float(np.max(self.X))
        self.norm_const = max(self.x_max, 1.0)
        if y_transform not in ("asinh", "signed_log", None, "none"):
            raise ValueError(y_transform)
        self.y_transform = y_transform
        if y_transform_scale is None:
            self.y_scale = float(np.percentile(np.abs(self.Y), y_transform_percentile)) if y_transform_percentile is not None else 1.0
        else:
            self.y_scale = float(y_transform_scale)
        explicit = (min_y is not None) and (max_y is not None)
        if explicit:
            self.min_vel, self.max_vel = float(min_y), float(max_y)
            self.trans_min = float(self._fwd(np.float64(self.min_vel)))
            self.trans_max = float(self._fwd(np.float64(self.max_vel)))
        else:
            self.min_vel = float(np.percentile(self.Y, lower_percentile))
            self.max_vel = float(np.percentile(self.Y, upper_percentile))
            yt = self._fwd(self.Y)
            self.trans_min = float(np.percentile(yt, lower_percentile))
            self.trans_max = float(np.percentile(yt, upper_percentile))
        if self.trans_max == self.trans_min:
            self.trans_max = self.trans_min + 1.0
        self.clip_outliers = clip_outliers

    def _fwd(self, arr):
        if self.y_transform == "asinh":
            return np.arcsinh(arr / self.y_scale)
        if self.y_transform == "signed_log":
            return np.sign(arr) * np.log1p(np.abs(arr) / self.y_scale)
        return arr

    def __len__(self):
        return self.N

    def __getitem__(self, idx):
        x = torch.from_numpy(self.X[idx])
        mask = (x[:, 0:1] > 1.1).float()
        x = x / self.norm_const
        y_raw = self.Y[idx]
        if self.clip_outliers:
            y_raw = np.clip(y_raw, self.min_vel, self.max_vel)
        y_scaled = (2 * (self._fwd(y_raw) - self.trans_min) / (self.trans_max - self.trans_min) - 1.0).astype(np.float32)
        return x, torch.from_numpy(y_scaled), mask

    def denormalize(self, y_norm):
        if isinstance(y_norm, torch.Tensor):
            yt = (y_norm + 1.0) / 2.0 * (self.trans_max - self.trans_min) + self.trans_min
            if self.y_transform == "asinh":
                return torch.sinh(yt) * self.y_scale
            if self.y_transform == "signed_log":
                return torch.sign(yt) * torch.expm1(yt.abs()) * self.y_scale
            return yt
        yt = (y_norm + 1.0) / 2.0 * (self.trans_max - self.trans_min) + self.trans_min
        if self.y_transform == "asinh":
            return np.sinh(yt) * self.y_scale
        if self.y_transform == "signed_log":
            return np.sign(yt) * (np.expm1(np.abs(yt)) * self.y_scale)
        return yt


VEC_MAX = 4          # UCLSTM_VEC_MAX: target channels of the vector data path (the head kernels' limit on output channels)
_AXES = ("+w", "-w", "+h", "-h", None)


def _per_channel(v, Cy: int, what: str):
    """A scalar or one value per channel -> a list of ``Cy`` values (None stays None for every channel)."""
    if v is None or np.ndim(v) == 0:
        return [v] * Cy
    v = list(v)
    if len(v) != Cy:
        raise ValueError(f"VectorNPZDataset: {what} must be a scalar or one value per channel ({Cy}), got {len(v)}")
    return v


class VectorNPZDataset(NPZSequenceDataset):
    """``NPZSequenceDataset`` for a VECTOR target: ``Y [N,T,Cy,H,W]`` with ``1 <= Cy <= 4`` channels (the reference's ``u_map``,
    ``v_map``, ``w_map``, preprocessing/build_WVU_maps.py:162), each with normalisation constants of its own: ``y_scale``,
    ``min_vel``, ``max_vel``, ``trans_min``, ``trans_max`` are float64 arrays ``[Cy]`` (``x_max`` / ``norm_const`` stay scalars).
    Channel ``c``'s constants equal those of ``NPZSequenceDataset`` built with the same arguments on ``Y[:, :, c:c+1]``, and
    channel ``c`` of an item's ``y`` equals that dataset's ``y``, bit for bit.  ``min_y``, ``max_y`` and ``y_transform_scale``
    take a scalar or one value per channel.

    ``axes``: one entry per channel saying how it turns with the image.  ``"+w"`` / ``"-w"``: the component along image COLUMNS,
    positive towards increasing / decreasing column index; ``"+h"`` / ``"-h"``: the component along image ROWS; None: a scalar
    (such as ``w``).  At most one w-channel and one h-channel.  ``u`` east, ``v`` north on rows that run south:
    ``("+w", "-h", None)``.  ``channel_map(code)`` says what a move of ``Augment`` does to the channels (a mirror negates the
    component across it, a transpose swaps the two), ``tta_affine(code)`` says it for NORMALISED values.

    ``tie_horizontal=True``: the w- and the h-channel share ONE set of constants, computed from both channels together (as
    ``NPZSequenceDataset`` on the two channels concatenated along ``N``): horizontal wind has one scale, and only with shared
    constants is a transpose an exact map between normalised values (``tta_affine``).

    A subclass of ``NPZSequenceDataset`` (``Subset``, ``random_split`` and ``DeviceSequenceLoader`` take it) that does not run its
    constructor; code that reads a constant as a scalar fails on the array."""

    def __init__(self, npz_path, axes, tie_horizontal=False, lower_percentile=0.00001, upper_percentile=99.99999, clip_outliers=True,
                 min_y=None, max_y=None, y_transform="asinh", y_transform_scale=None, y_transform_percentile=99):
        with np.load(npz_path, allow_pickle=False) as data:
            self.X = data["X"].astype(np.float32)
            self.Y = data["Y"].astype(np.float32)
        self.N, self.T, _, self.H, self.W = self.X.shape
        if self.Y.ndim != 5 or not 1 <= self.Y.shape[2] <= VEC_MAX:
            raise ValueError(f"VectorNPZDataset: Y must be [N,T,Cy,H,W] with 1 <= Cy <= {VEC_MAX}, got {self.Y.shape}")
        self.Cy = Cy = int(self.Y.shape[2])
        self.axes = tuple(axes)
        if len(self.axes) != Cy or any(a not in _AXES for a in self.axes):
            raise ValueError(f"VectorNPZDataset: axes must hold one of {_AXES} per target channel ({Cy}), got {axes!r}")
        w = [c for c, a in enumerate(self.axes) if a is not None and a[1] == "w"]
        h = [c for c, a in enumerate(self.axes) if a is not None and a[1] == "h"]
        if len(w) > 1 or len(h) > 1:
            raise ValueError(f"VectorNPZDataset: at most one w-channel and one h-channel, got {axes!r}")
        self.w_channel, self.h_channel = (w[0] if w else None), (h[0] if h else None)
        self.tie_horizontal = bool(tie_horizontal)
        self.x_max = float(np.max(self.X))
        self.norm_const = max(self.x_max, 1.0)
        if y_transform not in ("asinh", "signed_log", None, "none"):
            raise ValueError(y_transform)
        self.y_transform, self.clip_outliers = y_transform, clip_outliers
        lo, hi, sc = (_per_channel(v, Cy, n) for v, n in ((min_y, "min_y"), (max_y, "max_y"), (y_transform_scale, "y_transform_scale")))
        tied = (self.w_channel, self.h_channel) if self.tie_horizontal and w and h else ()
        names = ("y_scale", "min_vel", "max_vel", "trans_min", "trans_max")
        for name in names:
            setattr(self, name, np.zeros(Cy, dtype=np.float64))
        shared = None
        for c in range(Cy):
            if c in tied:
                if shared is None:
                    both = np.concatenate([self.Y[:, :, k:k + 1] for k in tied], axis=0)
                    shared = self._constants(both, lo[c], hi[c], sc[c], lower_percentile, upper_percentile, y_transform_percentile)
                vals = shared
            else:
                vals = self._constants(self.Y[:, :, c:c + 1], lo[c], hi[c], sc[c], lower_percentile, upper_percentile,
                                       y_transform_percentile)
            for name, v in zip(names, vals):
                getattr(self, name)[c] = v

    def _fwd_with(self, arr, y_scale):
        if self.y_transform == "asinh":
            return np.arcsinh(arr / y_scale)
        if self.y_transform == "signed_log":
            return np.sign(arr) * np.log1p(np.abs(arr) / y_scale)
        return arr

    def _fwd(self, arr):
        raise TypeError("VectorNPZDataset has one transform scale per channel: there is no scalar _fwd")

    def _constants(self, Y, min_y, max_y, y_transform_scale, lower_percentile, upper_percentile, y_transform_percentile):
        """The constants ``NPZSequenceDataset.__init__`` derives from the one-channel array ``Y``, statement for statement."""
        if y_transform_scale is None:
            y_scale = float(np.percentile(np.abs(Y), y_transform_percentile)) if y_transform_percentile is not None else 1.0
        else:
            y_scale = float(y_transform_scale)
        if (min_y is not None) and (max_y is not None):
            min_vel, max_vel = float(min_y), float(max_y)
            trans_min = float(self._fwd_with(np.float64(min_vel), y_scale))
            trans_max = float(self._fwd_with(np.float64(max_vel), y_scale))
        else:
            min_vel = float(np.percentile(Y, lower_percentile))
            max_vel = float(np.percentile(Y, upper_percentile))
            yt = self._fwd_with(Y, y_scale)
            trans_min = float(np.percentile(yt, lower_percentile))
            trans_max = float(np.percentile(yt, upper_percentile))
        if trans_max == trans_min:
            trans_max = trans_min + 1.0
        return y_scale, min_vel, max_vel, trans_min, trans_max

    def __getitem__(self, idx):
        x = torch.from_numpy(self.X[idx])
        mask = (x[:, 0:1] > 1.1).float()
        x = x / self.norm_const
        y_raw = self.Y[idx]
        y = np.empty(y_raw.shape, dtype=np.float32)
        for c in range(self.Cy):                                   # NPZSequenceDataset.__getitem__ with channel c's Python floats
            v = y_raw[..., c, :, :]
            tmin, tmax = float(self.trans_min[c]), float(self.trans_max[c])
            if self.clip_outliers:
                v = np.clip(v, float(self.min_vel[c]), float(self.max_vel[c]))
            y[..., c, :, :] = (2 * (self._fwd_with(v, float(self.y_scale[c])) - tmin) / (tmax - tmin) - 1.0).astype(np.float32)
        return x, torch.from_numpy(y), mask

    def denormalize(self, y_norm):
        """``NPZSequenceDataset.denormalize`` with the per-channel constants broadcast along dim -3."""
        if np.ndim(y_norm) < 3 or y_norm.shape[-3] != self.Cy:
            raise ValueError(f"VectorNPZDataset.denormalize: dim -3 must hold the {self.Cy} target channels, got {tuple(y_norm.shape)}")
        if isinstance(y_norm, torch.Tensor):
            def col(a):
                return torch.as_tensor(a, dtype=y_norm.dtype if y_norm.is_floating_point() else torch.float64,
                                       device=y_norm.device).reshape(-1, 1, 1)
            tmin, tmax, scale = col(self.trans_min), col(self.trans_max), col(self.y_scale)
            yt = (y_norm + 1.0) / 2.0 * (tmax - tmin) + tmin
            if self.y_transform == "asinh":
                return torch.sinh(yt) * scale
            if self.y_transform == "signed_log":
                return torch.sign(yt) * torch.expm1(yt.abs()) * scale
            return yt
        tmin, tmax, scale = (a.reshape(-1, 1, 1) for a in (self.trans_min, self.trans_max, self.y_scale))
        if getattr(y_norm, "dtype", None) == np.float32:           # the scalar class keeps f32 arrays f32 (Python-float constants)
            tmin, tmax, scale = (a.astype(np.float32) for a in (tmin, tmax, scale))
        yt = (y_norm + 1.0) / 2.0 * (tmax - tmin) + tmin
        if self.y_transform == "asinh":
            return np.sinh(yt) * scale
        if self.y_transform == "signed_log":
            return np.sign(yt) * (np.expm1(np.abs(yt)) * scale)
        return yt

    def channel_map(self, code: int):
        """What the move ``code`` of ``Augment`` (``h | v << 1 | t << 2``, applied h, then v, then t) does to the channels: per
        OUTPUT channel ``(source channel, negate)``.  h negates the w-channel, v the h-channel; t lets the w-channel take the
        h-channel's plane and the reverse, both times ``s_w * s_h`` (the signs in ``axes``); scalars map to themselves.
        ``ValueError`` for a code with t when exactly one of the two horizontal channels exists."""
        code = int(code)
        if not 0 <= code <= 7:
            raise ValueError(f"code must be in 0..7, got {code}")
        w, h = self.w_channel, self.h_channel
        cur = [(c, False) for c in range(self.Cy)]
        if code & 1 and w is not None:
            cur[w] = (cur[w][0], not cur[w][1])
        if code & 2 and h is not None:
            cur[h] = (cur[h][0], not cur[h][1])
        if code & 4 and (w is not None or h is not None):
            if w is None or h is None:
                raise ValueError(f"VectorNPZDataset: a transpose swaps the w- and the h-channel, axes {self.axes!r} name only one")
            flip = self.axes[w][0] != self.axes[h][0]              # s_w * s_h == -1
            cur[w], cur[h] = (cur[h][0], cur[h][1] != flip), (cur[w][0], cur[w][1] != flip)
        return cur

    def chan_map_table(self) -> np.ndarray:
        """``channel_map`` of all eight codes as the kernels read it: int8 ``[8, Cy]``, bits 0-2 source channel, bit 7 negate.
        Codes with t are the identity where ``channel_map`` refuses them (the loader never sends such a code)."""
        tab = np.zeros((8, self.Cy), dtype=np.uint8)
        for code in range(8):
            try:
                cm = self.channel_map(code)
            except ValueError:
                cm = [(c, False) for c in range(self.Cy)]
            tab[code] = [src | (0x80 if neg else 0) for src, neg in cm]
        return tab.view(np.int8)

    def tta_affine(self, code: int):
        """The move ``code`` on NORMALISED values: per output channel ``(source channel, sign, offset)`` with
        ``out[c] = sign * move(y_n[source]) + offset``.  All three transforms are odd, so negating the physical value is
        ``y_n -> -y_n - 2 (trans_max + trans_min) / (trans_max - trans_min)`` (exact where nothing was clipped); a swap is exact
        only between channels with the same constants: ``ValueError`` otherwise (build the dataset with ``tie_horizontal=True``)."""
        out = []
        for c, (src, neg) in enumerate(self.channel_map(code)):
            if src != c and any(getattr(self, n)[src] != getattr(self, n)[c] for n in ("y_scale", "trans_min", "trans_max")):
                raise ValueError(f"VectorNPZDataset.tta_affine: code {code} swaps channels {src} and {c}, whose normalisation constants "
                                 "differ; build the dataset with tie_horizontal=True")
            tmin, tmax = float(self.trans_min[c]), float(self.trans_max[c])
            out.append((src, -1.0, -2.0 * (tmax + tmin) / (tmax - tmin)) if neg else (src, 1.0, 0.0))
        return out

    def target_consts(self):
        """``uclstm_target_consts [Cy]`` for the entry points (host memory, read at launch); built once."""
        from . import _lib as L
        arr = self.__dict__.get("_target_consts")
        if arr is None:
            arr = (L.TargetConsts * self.Cy)(*[L.TargetConsts(float(self.min_vel[c]), float(self.max_vel[c]), float(self.y_scale[c]),
                                                               float(self.trans_min[c]), float(self.trans_max[c])) for c in range(self.Cy)])
            self.__dict__["_target_consts"] = arr
        return arr


def _refuse_vector(ds, what: str):
    if isinstance(ds, VectorNPZDataset):
        raise TypeError(f"{what} does not take a vector dataset (VectorNPZDataset): it de-normalises with one scalar set of "
                        "constants; use VectorEvalReport / evaluate_vector_report, or evaluate(..., per_channel=True) for "
                        "per-component metrics")


def device_transform(ds, x_raw: torch.Tensor, y_raw: torch.Tensor):
    """``NPZSequenceDataset.__getitem__`` (train/unet.py:273-304) for a whole RAW batch already on the device:
    ``x_raw [B,T,C,H,W]``, ``y_raw [B,T,1,H,W]`` f32 -> ``(x, y, mask)`` exactly as the host dataset would yield them
    (every target transform of the dataset: ``asinh`` through ``uclstm_dataset_transform``, ``signed_log`` and none through
    ``uclstm_dataset_gather_transform`` in identity order).  One kernel; lets a loader ship raw ``.npz`` slabs and skip the
    per-item numpy work -- ``DeviceSequenceLoader`` below keeps the whole raw dataset on the device instead."""
    from . import _lib as L
    x_raw = ops._dev(x_raw.contiguous(), torch.float32, "x_raw")
    y_raw = ops._dev(y_raw.contiguous(), torch.float32, "y_raw")
    if isinstance(ds, VectorNPZDataset):   # y_raw [B,T,Cy,H,W]: the vector gather over the batch itself, identity order, no remap
        return _gather_vec(ds, x_raw, y_raw, None, None, x_raw.shape[0], (x_raw.shape[1],) + tuple(x_raw.shape[3:]), 2)
    if ds.y_transform != "asinh":          # 'signed_log' / None: the gather kernel over the batch itself, identity order
        return _gather_transform(ds, x_raw, y_raw, None, x_raw.shape[0])
    B, T, Cc, H, W = x_raw.shape
    x, y = torch.empty_like(x_raw), torch.empty_like(y_raw)
    mask = torch.empty_like(y_raw)
    L.check(L.lib.uclstm_dataset_transform(ops._p(x_raw), ops._p(y_raw), ops._p(x), ops._p(y), ops._p(mask), B * T, Cc, H * W,
                                           float(ds.norm_const), float(ds.min_vel), float(ds.max_vel), int(bool(ds.clip_outliers)),
                                           float(ds.y_scale), float(ds.trans_min), float(ds.trans_max), ops._stream()),
            "dataset_transform")
    return x, y, mask


def _gather_out(x_all, n_out, shape, Cy, out):
    """The ``(x, y, mask)`` a gather writes: the caller-owned ``out``, or fresh tensors ``[n_out, T_out, C | Cy | 1, Ho, Wo]`` on the
    current stream for ``shape = (T_out, Ho, Wo)``."""
    if out is not None:
        x, y, mask = out
        return x, y, mask
    To, Ho, Wo = shape
    return tuple(torch.empty((n_out, To, c, Ho, Wo), dtype=torch.float32, device=x_all.device) for c in (x_all.shape[2], Cy, 1))


def _aug_table(aug, n_out, who):
    """The device table of a gather with a remap: int32 ``[>= n_out, 4]`` rows ``{code, oy, ox, t0}``."""
    from . import _lib as L
    aug = ops._dev(aug, torch.int32, "aug")
    if aug.dim() != 2 or aug.shape[1] != 4 or aug.shape[0] < n_out:
        raise L.UclstmError(f"{who}: aug must be int32 [>= {n_out}, 4], got {tuple(aug.shape)}")
    return aug


def _gather_transform(ds, x_all, y_all, idx, n_out, out=None):
    """One launch of ``uclstm_dataset_gather_transform``: the sequences ``idx[0..n_out)`` (device int64; None = the first
    ``n_out`` in order) of the RAW device arrays ``x_all [N,T,C,H,W]`` / ``y_all [N,T,1,H,W]`` as ``ds.__getitem__`` would yield
    them.  ``out``: caller-owned ``(x, y, mask)`` to write into; fresh tensors on the current stream otherwise."""
    from . import _lib as L
    N, T, Cc, H, W = x_all.shape
    x, y, mask = _gather_out(x_all, n_out, (T, H, W), 1, out)
    L.check(L.lib.uclstm_dataset_gather_transform(
        ops._p(x_all), ops._p(y_all), ops._p(idx), N, n_out, T, Cc, H * W, ops._p(x), ops._p(y), ops._p(mask),
        _TRANSFORM_IDS[ds.y_transform], float(ds.norm_const), float(ds.min_vel), float(ds.max_vel), int(bool(ds.clip_outliers)),
        float(ds.y_scale), float(ds.trans_min), float(ds.trans_max), ops._stream()), "dataset_gather_transform")
    return x, y, mask


# ---------------------------------------------------------------------------------------------
# augmentation on the device: flips, transpose, crop, time window -- every one an index remap
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Augment:
    """What ``DeviceSequenceLoader(augment=...)`` draws per output sequence.  ``hflip`` / ``vflip`` / ``transpose``: each enabled
    bit of the code is Bernoulli(1/2) (``code = h | v << 1 | t << 2``; on a frame ``s``: ``flip(-1)`` for h, then ``flip(-2)`` for
    v, then ``transpose(-2, -1)`` for t -- together the eight elements of the dihedral group).  ``crop=(Ho, Wo)``: the OUTPUT
    frame size, cut at an offset uniform over the positions that are multiples of ``crop_align`` and keep the window inside the
    source (``crop_align=4`` keeps the kernel's 16-byte path when the widths are multiples of 4).  ``frames=T_out``: a window of
    ``T_out`` consecutive frames at a uniform start.  ``transpose`` needs a square output frame.

    The draw knows nothing about the target.  For a scalar target (the reference's ``MAP_TYPE = 'w'``) the remap is everything;
    the horizontal components of a vector target also change sign under mirrors and swap under transposes:
    ``DeviceSequenceLoader`` over a ``VectorNPZDataset`` does that with the dataset's ``axes`` (``uclstm_dataset_gather_vec``)."""
    hflip: bool = False
    vflip: bool = False
    transpose: bool = False
    crop: Optional[tuple] = None
    frames: Optional[int] = None
    crop_align: int = 1

    def __post_init__(self):
        if self.crop is not None:
            crop = tuple(int(v) for v in self.crop)
            if len(crop) != 2 or min(crop) <= 0:
                raise ValueError(f"Augment: crop must be (Ho, Wo) with positive sizes, got {self.crop!r}")
            object.__setattr__(self, "crop", crop)
            if self.transpose and crop[0] != crop[1]:
                raise ValueError(f"Augment: transpose needs a square output frame, got crop {crop}")
        if self.frames is not None and int(self.frames) <= 0:
            raise ValueError(f"Augment: frames must be positive, got {self.frames}")
        if int(self.crop_align) < 1:
            raise ValueError(f"Augment: crop_align must be at least 1, got {self.crop_align}")

    @property
    def code_mask(self) -> int:
        return int(bool(self.hflip)) | int(bool(self.vflip)) << 1 | int(bool(self.transpose)) << 2

    def output_shape(self, T: int, H: int, W: int):
        """``(T_out, Ho, Wo)`` for a source of ``T`` frames of ``H x W``; ``ValueError`` when it does not fit."""
        Ho, Wo = self.crop if self.crop is not None else (H, W)
        To = T if self.frames is None else int(self.frames)
        if Ho > H or Wo > W or To > T:
            raise ValueError(f"Augment: output of {To} frames of {Ho} x {Wo} does not fit a source of {T} frames of {H} x {W}")
        if self.transpose and Ho != Wo:
            raise ValueError(f"Augment: transpose needs a square output frame, got {Ho} x {Wo}")
        return To, Ho, Wo


def d4_inverse(code: int) -> int:
    """The code that undoes ``code``: a code without t is its own inverse; with t the h and v bits swap."""
    code = int(code)
    if not 0 <= code <= 7:
        raise ValueError(f"code must be in 0..7, got {code}")
    return code if not code & 4 else 4 | (code & 1) << 1 | (code & 2) >> 1


def epoch_augment(n: int, T: int, H: int, W: int, augment: Augment, generator=None) -> np.ndarray:
    """The table of one epoch: int32 ``[n, 4]`` rows ``{code, oy, ox, t0}``, one per output sequence -- a pure function of its
    arguments and the generator's state.  Drawn with ``torch.randint(..., generator=generator)`` on the CPU in this order: all
    codes (uniform over 0..7, masked to the enabled bits), then all ``oy``, then all ``ox``, then all ``t0``; a column with a
    single possible value (a disabled option, a crop as large as the source) is zero and draws nothing.  So a seeded generator
    reproduces an epoch, and the next call continues the stream."""
    To, Ho, Wo = augment.output_shape(T, H, W)
    n, align = int(n), int(augment.crop_align)
    tab = np.zeros((n, 4), dtype=np.int32)
    if n <= 0:
        return tab

    def draw(count):
        return torch.randint(0, count, (n,), generator=generator).numpy().astype(np.int32)
    if augment.code_mask:
        tab[:, 0] = draw(8) & augment.code_mask
    for col, count, step in ((1, (H - Ho) // align + 1, align), (2, (W - Wo) // align + 1, align), (3, T - To + 1, 1)):
        if count > 1:
            tab[:, col] = draw(count) * step
    return tab


def _gather_augment(ds, x_all, y_all, idx, aug, n_out, shape, flags, out=None):
    """One launch of ``uclstm_dataset_gather_augment``: ``_gather_transform`` with the per-sequence remap of the device table
    ``aug`` (int32 ``[n_out, 4]`` rows ``{code, oy, ox, t0}``).  ``shape = (T_out, Ho, Wo)`` of the output; ``flags``: bit 0 = the
    table may hold codes with t, bit 1 = every ``ox`` is a multiple of 4.  Bit-identical to ``_gather_transform`` of the same
    rows moved with ``torch.flip`` / ``transpose`` / slicing."""
    from . import _lib as L
    N, T, Cc, H, W = x_all.shape
    To, Ho, Wo = (int(v) for v in shape)
    aug = _aug_table(aug, n_out, "_gather_augment")
    x, y, mask = _gather_out(x_all, n_out, (To, Ho, Wo), 1, out)
    L.check(L.lib.uclstm_dataset_gather_augment(
        ops._p(x_all), ops._p(y_all), ops._p(idx), ops._p(aug), N, n_out, T, To, Cc, H, W, Ho, Wo, int(flags),
        ops._p(x), ops._p(y), ops._p(mask), _TRANSFORM_IDS[ds.y_transform], float(ds.norm_const), float(ds.min_vel),
        float(ds.max_vel), int(bool(ds.clip_outliers)), float(ds.y_scale), float(ds.trans_min), float(ds.trans_max), ops._stream()),
        "dataset_gather_augment")
    return x, y, mask


def _gather_vec(ds, x_all, y_all, idx, aug, n_out, shape, flags, out=None):
    """One launch of ``uclstm_dataset_gather_vec`` for a ``VectorNPZDataset``: ``_gather_augment`` with ``y_all [N,T,Cy,H,W]`` ->
    ``y [n_out,T_out,Cy,Ho,Wo]``, the channels moved by ``ds.chan_map_table()`` and normalised with their own constants.
    ``aug=None``: no remap (the plain gather; ``shape`` is then the source's)."""
    from . import _lib as L
    N, T, Cc, H, W = x_all.shape
    Cy = ds.Cy
    To, Ho, Wo = (int(v) for v in shape)
    if y_all.dim() != 5 or y_all.shape[2] != Cy or y_all.shape[:2] != x_all.shape[:2] or y_all.shape[3:] != x_all.shape[3:]:
        raise L.UclstmError(f"_gather_vec: y must be [{N},{T},{Cy},{H},{W}] beside x {tuple(x_all.shape)}, got {tuple(y_all.shape)}")
    if aug is not None:
        aug = _aug_table(aug, n_out, "_gather_vec")
    x, y, mask = _gather_out(x_all, n_out, (To, Ho, Wo), Cy, out)
    table = ds.__dict__.get("_chan_map_host")
    if table is None:
        table = ds.__dict__["_chan_map_host"] = np.ascontiguousarray(ds.chan_map_table())
    L.check(L.lib.uclstm_dataset_gather_vec(
        ops._p(x_all), ops._p(y_all), ops._p(idx), ops._p(aug), N, n_out, T, To, Cc, Cy, H, W, Ho, Wo, int(flags),
        table.ctypes.data, ops._p(x), ops._p(y), ops._p(mask), _TRANSFORM_IDS[ds.y_transform], float(ds.norm_const),
        int(bool(ds.clip_outliers)), ds.target_consts(), ops._stream()), "dataset_gather_vec")
    return x, y, mask


def _plane_args(who, t, code, fits, need, out, accumulate):
    """What ``plane_d4`` and ``plane_d4_vec`` check alike: ``t`` (f32, contiguous, on the device, of a shape that ``fits``, which
    ``need`` puts into words), the code, and ``out``: the moved shape on ``t``'s device and not ``t`` itself, or None = a fresh
    tensor (refused with ``accumulate``).  Returns ``(t, code, out)``."""
    code = int(code)
    t = ops._dev(t, torch.float32, f"{who} input")
    if not fits(t) or not 0 <= code <= 7:
        raise ValueError(f"{who}: {need} and a code in 0..7 are required, got {tuple(t.shape)}, code {code}")
    H, W = t.shape[-2:]
    shape = tuple(t.shape[:-2]) + ((W, H) if code & 4 else (H, W))
    if out is None:
        if accumulate:
            raise ValueError(f"{who}: accumulate=True needs out=")
        out = torch.empty(shape, dtype=torch.float32, device=t.device)
    else:
        ops._dev(out, torch.float32, f"{who} out")
        if tuple(out.shape) != shape or out.device != t.device or out.data_ptr() == t.data_ptr():
            raise ValueError(f"{who}: out must be another tensor of shape {shape} on {t.device}, got {tuple(out.shape)} on {out.device}")
    return t, code, out


def plane_d4(t: torch.Tensor, code: int, out: Optional[torch.Tensor] = None, accumulate: bool = False, scale: float = 1.0):
    """Move the last two dims of the contiguous f32 device tensor ``t`` by ``code`` (0..7, as in ``Augment``):
    ``out = (accumulate ? out : 0) + scale * move(t)``, one launch of ``uclstm_plane_d4``.  ``out``: ``t``'s shape, with the last
    two dims swapped for codes with t; a fresh tensor when None (then ``accumulate`` is refused).  ``out`` must not be ``t``."""
    from . import _lib as L
    t, code, out = _plane_args("plane_d4", t, code, lambda t: t.dim() >= 2, "a tensor of at least 2 dims", out, accumulate)
    H, W = t.shape[-2:]
    if t.numel():
        L.check(L.lib.uclstm_plane_d4(ops._p(t), ops._p(out), t.numel() // (H * W), H, W, code, int(bool(accumulate)), float(scale),
                                      ops._stream()), "plane_d4")
    return out


def plane_d4_vec(t: torch.Tensor, code: int, affine, out: Optional[torch.Tensor] = None, accumulate: bool = False, scale: float = 1.0):
    """``plane_d4`` for frames of channels that turn with the image: ``t [..., Cy, H, W]``, ``affine`` = per output channel
    ``(source channel, sign, offset)`` as ``VectorNPZDataset.tta_affine`` returns it, and
    ``out[..., c, :, :] = (accumulate ? out : 0) + scale * (sign * move(t[..., source, :, :]) + offset)``: one launch of
    ``uclstm_plane_d4_vec``."""
    from . import _lib as L
    affine = list(affine)
    Cy = len(affine)
    t, code, out = _plane_args("plane_d4_vec", t, code, lambda t: t.dim() >= 3 and t.shape[-3] == Cy and 1 <= Cy <= VEC_MAX,
                               f"a tensor [..., {Cy}, H, W] with 1 <= Cy <= {VEC_MAX}", out, accumulate)
    if any(not 0 <= int(src) < Cy or sign not in (1, -1) for src, sign, _ in affine):
        raise ValueError(f"plane_d4_vec: affine must hold (source channel in [0, {Cy}), sign +-1, offset) per channel, got {affine}")
    H, W = t.shape[-2:]
    if t.numel():
        import ctypes as C
        cmap = (C.c_int8 * Cy)(*[(int(src) | (0x80 if sign < 0 else 0)) - (256 if sign < 0 else 0) for src, sign, _ in affine])
        offs = (C.c_float * Cy)(*[float(off) for _, _, off in affine])
        L.check(L.lib.uclstm_plane_d4_vec(ops._p(t), ops._p(out), t.numel() // (Cy * H * W), Cy, H, W, code, C.addressof(cmap),
                                          C.addressof(offs), int(bool(accumulate)), float(scale), ops._stream()), "plane_d4_vec")
    return out


_TTA_SETS = {"flips": (0, 1, 2, 3), "d4": tuple(range(8))}


@torch.no_grad()
def predict_tta(model, x: torch.Tensor, codes="flips", state=None, dataset=None) -> torch.Tensor:
    """Test-time augmentation: the mean over ``codes`` of ``inverse move(model(move(x)))``, ``[B,T,C,H,W]`` f32.
    ``codes``: ``"flips"`` = (0, 1, 2, 3), ``"d4"`` = all eight, or an iterable of codes.  For each code in the given order: ``x``
    is moved with ``plane_d4``, the model runs under ``no_grad``, its frames are stacked as the epoch loops stack them, and the
    output moved by the INVERSE code is accumulated with weight 1 / len(codes) by the same kernel (left to right in f32).
    ``model`` is anything that returns ``(frames or tensor, state)``.  Codes with t need square frames.

    ``dataset``: a ``VectorNPZDataset`` whose target channels the model predicts (normalised).  The inputs move as before; the
    outputs come back through ``plane_d4_vec`` with ``dataset.tta_affine(d4_inverse(c))``, so a horizontal component changes sign
    and channel with the frame (codes with t need ``tie_horizontal=True``).  None: scalar outputs, the launches as they were."""
    if isinstance(codes, str):
        if codes not in _TTA_SETS:
            raise ValueError(f"predict_tta: codes must be one of {sorted(_TTA_SETS)} or an iterable of codes, got {codes!r}")
        codes = _TTA_SETS[codes]
    codes = tuple(int(c) for c in codes)
    if not codes or any(not 0 <= c <= 7 for c in codes):
        raise ValueError(f"predict_tta: codes must be a non-empty sequence of values in 0..7, got {codes}")
    if any(c & 4 for c in codes) and x.shape[-1] != x.shape[-2]:
        raise ValueError(f"predict_tta: codes with a transpose need square frames, got {x.shape[-2]} x {x.shape[-1]}")
    if dataset is not None and not isinstance(dataset, VectorNPZDataset):
        raise TypeError(f"predict_tta: dataset must be a VectorNPZDataset or None, got {type(dataset).__name__}")
    affine = None if dataset is None else {c: dataset.tta_affine(d4_inverse(c)) for c in codes}      # raises before any launch
    x = x.contiguous().float()
    acc = None
    for c in codes:
        xc = plane_d4(x, c)
        output, _ = model(xc) if state is None else model(xc, state)
        y = _stack(output).contiguous().float()
        if affine is not None:
            acc = plane_d4_vec(y, d4_inverse(c), affine[c], out=acc, accumulate=acc is not None, scale=1.0 / len(codes))
        elif acc is None:
            acc = plane_d4(y, d4_inverse(c), scale=1.0 / len(codes))
        else:
            plane_d4(y, d4_inverse(c), out=acc, accumulate=True, scale=1.0 / len(codes))
    return acc


def _root_rows(dataset):
    """``dataset`` (an ``NPZSequenceDataset`` or nested ``Subset``s of one, as ``random_split`` returns them) ->
    ``(root dataset, rows)``: ``rows[p]`` is the root's row behind position ``p`` (int64 array; None = identity)."""
    rows, d = None, dataset
    while isinstance(d, torch.utils.data.Subset):
        ind = _checked(np.asarray(d.indices, dtype=np.int64).reshape(-1), len(d.dataset), "Subset index")
        rows = ind if rows is None else ind[rows]
        d = d.dataset
    if not isinstance(d, NPZSequenceDataset):
        raise TypeError(f"DeviceSequenceLoader needs an NPZSequenceDataset or a Subset of one, got {type(d).__name__}")
    return d, rows


def _checked(ind: np.ndarray, n: int, what: str) -> np.ndarray:
    bad = (ind < 0) | (ind >= n)
    if bad.any():
        raise IndexError(f"{what} {int(ind[bad][0])} is outside [0, {n})")
    return ind


def epoch_rows(dataset, sampler, batch_size: int, drop_last: bool = False):
    """The batches of one epoch as rows of the ROOT dataset: a pure function of its arguments (plus the sampler's own random
    state).  ``sampler`` yields positions into ``dataset`` (any torch sampler or iterable; None = in order); they are chunked as
    ``torch.utils.data.BatchSampler`` chunks them and mapped through the Subset indices.  Returns a list of int64 arrays.
    A position or row out of range raises ``IndexError``."""
    if batch_size <= 0:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    root, rows = _root_rows(dataset)
    pos = np.arange(len(dataset), dtype=np.int64) if sampler is None else np.fromiter((int(p) for p in sampler), dtype=np.int64)
    pos = _checked(pos, len(dataset), "sampler position")
    flat = _checked(pos if rows is None else rows[pos], len(root), "dataset row")
    stop = len(flat) // batch_size * batch_size if drop_last else len(flat)
    return [flat[s:min(s + batch_size, stop)] for s in range(0, stop, batch_size)]


class DeviceSequenceLoader:
    """``DataLoader(dataset, batch_size, ...)`` for a dataset whose RAW arrays live on the GPU: a batch is one launch of
    ``uclstm_dataset_gather_transform`` (gather by row, mask, normalise, clip, target transform) instead of per-item numpy
    work, a collate and a host-to-device copy.  Yields ``(x [b,T,C,H,W], y [b,T,1,H,W], mask [b,T,1,H,W])`` as fresh f32 device
    tensors on the current stream, batch for batch what a ``DataLoader`` over the same sampler yields;
    ``train_one_epoch`` / ``evaluate`` / ``evaluate_report`` take it unchanged.

    ``dataset``: an ``NPZSequenceDataset`` or (nested) ``Subset``s of one.  Its raw ``X`` / ``Y`` are uploaded once per
    (dataset, device) and cached on the dataset object, so loaders over several Subsets of one dataset share one device copy;
    a dataset larger than ``max_resident_bytes`` (default: 80 % of the device memory free at that moment) raises
    ``UclstmError`` -- streaming is not implemented.  The index order is the torch sampler's, iterated on the host:
    ``sampler=`` any sampler or iterable of positions (``DistributedSampler``: ``set_epoch`` stays the caller's job),
    ``shuffle=True`` = ``RandomSampler(dataset, generator=generator)``.  Per epoch the row list goes to the device as one pinned
    int64 tensor; per batch nothing is copied and nothing synchronises.

    ``augment=Augment(...)``: every output sequence is flipped / transposed / cropped / cut in time on the way, by one launch of
    ``uclstm_dataset_gather_augment`` per batch instead (batches are then ``[b, T_out, C, Ho, Wo]``).  Per epoch
    ``epoch_augment`` draws one table row per POSITION from ``augment_generator`` (two positions that name the same row get
    independent draws); the table is uploaded once next to the row list, and ``last_augment`` keeps the host copy of the current
    epoch.  A batch is bit-identical to the plain batch moved with ``torch.flip`` / ``transpose`` / slicing.
    ``augment=None`` is the plain path, launch for launch.

    A ``VectorNPZDataset`` (or Subsets of one) yields ``y [b,T_out,Cy,Ho,Wo]`` through ``uclstm_dataset_gather_vec``, with or
    without ``augment``: the move also negates and swaps the horizontal components as the dataset's ``axes`` say
    (``channel_map``, a host table: nothing more is uploaded), and every channel is normalised with its own constants.
    ``Augment(transpose=True)`` over a dataset with only one horizontal channel is refused at construction.  A scalar dataset
    takes the entry points it always took."""

    def __init__(self, dataset, batch_size: int, shuffle: bool = False, sampler=None, drop_last: bool = False, generator=None,
                 device="cuda", max_resident_bytes: Optional[int] = None, augment: Optional[Augment] = None, augment_generator=None):
        self.root, _ = _root_rows(dataset)
        if batch_size <= 0:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if sampler is not None and shuffle:
            raise ValueError("sampler option is mutually exclusive with shuffle")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.L.UclstmError(f"DeviceSequenceLoader: a HIP device is required, got {dev} (this package has no CPU path)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        self.dataset, self.batch_size, self.drop_last = dataset, int(batch_size), bool(drop_last)
        if sampler is None:
            sampler = (torch.utils.data.RandomSampler(dataset, generator=generator) if shuffle
                       else torch.utils.data.SequentialSampler(dataset))
        self.sampler = sampler
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError(f"DeviceSequenceLoader: augment must be an Augment or None, got {type(augment).__name__}")
        self.augment, self.augment_generator, self.last_augment = augment, augment_generator, None
        if augment is not None:
            augment.output_shape(self.root.T, self.root.H, self.root.W)          # a crop that does not fit fails here, not mid-epoch
        self.vector = isinstance(self.root, VectorNPZDataset)
        if self.vector and augment is not None and augment.transpose:
            self.root.channel_map(4)                                             # an unpaired horizontal channel: ValueError here
        if self.vector:                                     # one entry point with or without augmentation (aug = NULL)
            self._gather = _gather_vec
        elif augment is not None:
            self._gather = _gather_augment
        else:
            self._gather = lambda ds, x_all, y_all, idx, aug, n_out, shape, flags, out: _gather_transform(ds, x_all, y_all, idx, n_out, out)
        self.x_all, self.y_all = self._resident(self.root, self.device, max_resident_bytes)

    @staticmethod
    def _resident(root, device, max_resident_bytes):
        cache = root.__dict__.setdefault("_device_resident", {})
        if device not in cache:
            need = int(root.X.nbytes) + int(root.Y.nbytes)
            limit = int(0.8 * torch.cuda.mem_get_info(device)[0]) if max_resident_bytes is None else int(max_resident_bytes)
            if need > limit:
                raise ops.L.UclstmError(f"DeviceSequenceLoader: the raw dataset needs {need} bytes on {device} "
                                        f"(X {root.X.nbytes} + Y {root.Y.nbytes}), the limit is {limit} bytes; "
                                        "streaming a dataset that does not fit is not implemented")
            cache[device] = (torch.from_numpy(np.ascontiguousarray(root.X)).to(device),
                             torch.from_numpy(np.ascontiguousarray(root.Y)).to(device))
        return cache[device]

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        return self.batches()

    def batches(self, out=None):
        """The epoch's batches.  ``out=(x, y, mask)``: every (full) batch is written into these caller-owned contiguous f32
        device buffers, which are yielded themselves -- the static inputs of a ``GraphedTrainStep``; a short last batch cannot
        be written into them, so ``drop_last=False`` is refused when the sampler's length is no multiple of the batch.  With
        ``augment`` the buffers have the OUTPUT shape ``(b, T_out, C, Ho, Wo)``."""
        T, Cc, H, W = self.x_all.shape[1:]
        if self.augment is not None:
            T, H, W = self.augment.output_shape(T, H, W)
        if out is not None:
            if not self.drop_last and len(self.sampler) % self.batch_size:
                raise ValueError(f"batches(out=...): the last batch of {len(self.sampler)} positions in batches of "
                                 f"{self.batch_size} would be short; use drop_last=True")
            Cy = self.root.Cy if self.vector else 1
            want = ((self.batch_size, T, Cc, H, W), (self.batch_size, T, Cy, H, W), (self.batch_size, T, 1, H, W))
            if len(out) != 3:
                raise ValueError("batches(out=...): expected (x, y, mask)")
            for t, shape, what in zip(out, want, ("out x", "out y", "out mask")):
                ops._dev(t, torch.float32, what)
                if tuple(t.shape) != shape or t.device != self.device:
                    raise ValueError(f"batches(out=...): {what} must be {shape} on {self.device}, got {tuple(t.shape)} on {t.device}")
        batches = epoch_rows(self.dataset, self.sampler, self.batch_size, self.drop_last)      # validated before any upload
        return self._run(batches, out)

    def _run(self, batches, out):
        if not batches:
            return
        # ONE pinned int64 tensor per epoch, copied without blocking; this generator's frame keeps it alive until the epoch ends
        pinned = torch.from_numpy(np.concatenate(batches)).pin_memory()
        rows = pinned.to(self.device, non_blocking=True)
        T, _, H, W = self.x_all.shape[1:]
        shape, flags, aug = (T, H, W), 2, None
        if self.augment is not None:
            shape = self.augment.output_shape(T, H, W)
            self.last_augment = epoch_augment(len(pinned), T, H, W, self.augment, self.augment_generator)
            flags = int(bool(self.augment.transpose)) | (0 if (self.last_augment[:, 2] % 4).any() else 2)
            pinned_aug = torch.from_numpy(self.last_augment).pin_memory()          # kept alive like the rows
            aug = pinned_aug.to(self.device, non_blocking=True)
        s = 0
        for b in [len(b) for b in batches]:
            yield self._gather(self.root, self.x_all, self.y_all, rows[s:s + b], None if aug is None else aug[s:s + b], b, shape, flags, out)
            s += b
        del pinned


# ---------------------------------------------------------------------------------------------
# dataset statistics on the device: order statistics by radix select, extremes, the dataset's normalisation constants
# ---------------------------------------------------------------------------------------------
SELECT_MAX_LAUNCH = 1 << 30          # elements per uclstm_select_accumulate / uclstm_dataset_extremes call (the ABI takes n < 2^31)
_KIND_IDS = {"signed": 0, "abs": 1}


def _stat_pieces(t, what: str):
    """``t`` (an f32 device tensor, or a re-iterable of them standing for their concatenation) -> a callable that yields
    ``(data_ptr, n, keepalive)`` launches of at most ``SELECT_MAX_LAUNCH`` elements, anew on every call."""
    if isinstance(t, torch.Tensor):
        t = (t,)
    elif iter(t) is t:
        raise TypeError(f"{what}: the pieces are read once per pass, so a one-shot iterator cannot be used; "
                        "pass a list, a tuple or an object whose __iter__ starts over")

    def launches():
        for piece in t:
            piece = ops._dev(piece, torch.float32, what)
            n, step = piece.numel(), int(SELECT_MAX_LAUNCH)
            for off in range(0, n, step):          # an empty piece launches nothing
                yield piece.data_ptr() + 4 * off, min(step, n - off), piece
    return launches


def _stat_device(t) -> torch.device:
    if isinstance(t, torch.Tensor):
        return t.device
    if getattr(t, "device", None) is not None:
        return torch.device(t.device)
    for piece in t:
        return piece.device
    return torch.device("cuda", torch.cuda.current_device())


def _launch_select(t, ranks, kinds, what: str) -> torch.Tensor:
    """Every launch of one select over ``t``; returns the device int64 [8] result (words 0..3: out_info, words 4..7: the f32
    values) without synchronising."""
    import ctypes as C
    from . import _lib as L
    ranks, kinds = [int(r) for r in ranks], list(kinds)
    if not 1 <= len(ranks) <= L.SELECT_MAX_SLOTS or len(kinds) != len(ranks):
        raise ValueError(f"{what}: between 1 and {L.SELECT_MAX_SLOTS} ranks with one kind each are required, got {len(ranks)} and {len(kinds)}")
    for k in kinds:
        if k not in _KIND_IDS:
            raise ValueError(f"{what}: kind must be 'signed' or 'abs', got {k!r}")
    launches, device = _stat_pieces(t, what), _stat_device(t)
    with torch.cuda.device(device):
        ws = torch.empty(int(L.lib.uclstm_select_workspace_bytes()) // 8, dtype=torch.int64, device=device)
        out = torch.zeros(8, dtype=torch.int64, device=device)
        st = L.SelectState()
        c_ranks = (C.c_int64 * len(ranks))(*ranks)
        c_kinds = (C.c_int32 * len(ranks))(*[_KIND_IDS[k] for k in kinds])
        L.check(L.lib.uclstm_select_begin(C.byref(st), ops._p(ws), c_ranks, c_kinds, len(ranks), ops._stream()), "select_begin")
        for p in range(3):
            for ptr, n, _keep in launches():
                if ops.LAUNCH_LOG is not None:
                    ops.LAUNCH_LOG.append(("select", "accumulate", p, n))
                L.check(L.lib.uclstm_select_accumulate(C.byref(st), p, C.c_void_p(ptr), n, ops._stream()), "select_accumulate")
            L.check(L.lib.uclstm_select_narrow(C.byref(st), p, ops._stream()), "select_narrow")
        L.check(L.lib.uclstm_select_finish(C.byref(st), C.c_void_p(out.data_ptr() + 32), ops._p(out), ops._stream()), "select_finish")
    return out


def _read_select(out: torch.Tensor, n_slots: int):
    """The one host synchronisation of a select: ``(values f32 [n_slots], nan count, element count, out-of-range mask)``."""
    host = out.cpu().numpy()
    info = host[:4].view(np.uint64)
    return host[4:].view(np.float32)[:n_slots].copy(), int(info[0]), int(info[1]), int(info[2])


def device_order_statistics(t, ranks, kinds) -> np.ndarray:
    """Exact order statistics of f32 device data: ``values[i]`` is the element at index ``ranks[i]`` of the ascending order of
    the non-NaN elements of ``t`` (``kinds[i] == "signed"``) or of their absolute values (``"abs"``), as a float32 array; up to
    8 of them from ONE radix select (``uclstm_select_*``: three passes over the data for all ranks together, integer counts
    only, so the result does not depend on the run).  A zero comes back as +0.0.  ``t``: a contiguous f32 device tensor, or an
    iterable of them treated as one concatenated array -- it is iterated once per pass, so it must start over on every
    ``iter()`` (a list, or an object that uploads its chunks anew); a one-shot iterator is refused.  Tensors of more than
    ``SELECT_MAX_LAUNCH`` elements go to the kernel in several calls.  A rank outside ``[0, number of non-NaN elements)``
    raises ``IndexError``.  One host synchronisation, at the end."""
    values, _, count, bad = _read_select(_launch_select(t, ranks, kinds, "device_order_statistics"), len(list(kinds)))
    if bad:
        s = (bad & -bad).bit_length() - 1
        raise IndexError(f"device_order_statistics: rank {int(list(ranks)[s])} (slot {s}) is outside the non-NaN elements of an array of {count}")
    return values


def percentile_ranks(n: int, q: float, exact: bool = False):
    """``(lo, hi, gamma)`` of ``np.percentile(a, q)`` (method 'linear') for a float32 ``a`` of ``n`` elements: the two ranks it
    reads and the weight between them.  numpy forms the virtual index in the ARRAY's precision: ``f32(n-1) * (f32(q) / f32(100))``,
    so above 2^24 elements the rank itself is rounded -- reproduced here on purpose (parity with the host dataset).
    ``exact=True``: the same in f64, the true rank."""
    ft = np.float64 if exact else np.float32
    vi = ft(n - 1) * (ft(q) / ft(100))
    if vi >= ft(n - 1):
        lo = hi = n - 1
        prev = -1                       # numpy's index of "the last element"; its gamma is formed from it (and multiplies a zero difference)
    else:
        lo = prev = int(np.floor(vi))
        hi = lo + 1
    return lo, hi, ft(np.float64(vi) - np.float64(prev))


def percentile_lerp(a, b, gamma):
    """numpy's interpolation between the two order statistics ``a <= b`` in their own precision:
    ``a + (b-a)*g``, and ``b - (b-a)*(1-g)`` when ``g >= 0.5``."""
    ft = type(gamma)
    a, b = ft(a), ft(b)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return b - d * (ft(1) - gamma) if gamma >= 0.5 else a + d * gamma


def device_percentile(t, q, absolute: bool = False, exact: bool = False):
    """``float(np.percentile(t.cpu().numpy(), q))`` (of ``np.abs(...)`` with ``absolute=True``) from the device, bit for bit:
    numpy's rank rule for float32 data (``percentile_ranks``) on two order statistics of one radix select.  ``q``: a number, or a
    sequence of up to 4 (a list is returned).  ``exact=True`` forms the rank and the interpolation in f64 instead -- numpy's own
    rank is rounded to f32 above 2^24 elements.  NaN if the data holds a NaN, as numpy.  ``t`` as in
    ``device_order_statistics``.  One host synchronisation, at the end."""
    qs = [float(q)] if np.isscalar(q) else [float(v) for v in q]
    if not qs or len(qs) > 4 or any(not 0.0 <= v <= 100.0 for v in qs):
        raise ValueError(f"device_percentile: between 1 and 4 percentiles in [0, 100] are required, got {q!r}")
    launches = _stat_pieces(t, "device_percentile")
    n = sum(m for _, m, _ in launches())
    if n == 0:
        raise ValueError("device_percentile: the data is empty")
    rk = [percentile_ranks(n, v, exact) for v in qs]
    kind = "abs" if absolute else "signed"
    values, nan, _, _ = _read_select(_launch_select(t, [r for lo, hi, _ in rk for r in (lo, hi)], [kind] * (2 * len(qs)), "device_percentile"),
                                     2 * len(qs))
    res = [float("nan") if nan else float(percentile_lerp(values[2 * i], values[2 * i + 1], g)) for i, (_, _, g) in enumerate(rk)]
    return res[0] if np.isscalar(q) else res


def _key_value(k: int) -> float:
    k = int(k) & 0xffffffff
    return float(np.array([k ^ 0x80000000 if k & 0x80000000 else ~k & 0xffffffff], dtype=np.uint32).view(np.float32)[0])


def _launch_extremes(t, what: str) -> torch.Tensor:
    from . import _lib as L
    import ctypes as C
    launches, device = _stat_pieces(t, what), _stat_device(t)
    with torch.cuda.device(device):
        out = torch.empty(L.EXTREMES_WORDS, dtype=torch.int64, device=device)
        L.check(L.lib.uclstm_dataset_extremes_begin(ops._p(out), ops._stream()), "dataset_extremes_begin")
        for ptr, n, _keep in launches():
            if ops.LAUNCH_LOG is not None:
                ops.LAUNCH_LOG.append(("extremes", n))
            L.check(L.lib.uclstm_dataset_extremes(C.c_void_p(ptr), n, ops._p(out), ops._stream()), "dataset_extremes")
    return out


def _read_extremes(out: torch.Tensor) -> dict:
    from . import _lib as L
    w = out.cpu().numpy().view(np.uint64)
    some = int(w[L.EXTREMES_MIN_KEY]) <= int(w[L.EXTREMES_MAX_KEY])
    return {"min": _key_value(w[L.EXTREMES_MIN_KEY]) if some else float("nan"),
            "max": _key_value(w[L.EXTREMES_MAX_KEY]) if some else float("nan"),
            "nan_count": int(w[L.EXTREMES_NAN]), "nonzero": int(w[L.EXTREMES_NONZERO]), "count": int(w[L.EXTREMES_COUNT])}


def device_extremes(t) -> dict:
    """``{"min", "max", "nan_count", "nonzero", "count"}`` of f32 device data in one pass (``uclstm_dataset_extremes``): min and
    max ignore NaNs (NaN when there is no other element; a zero is +0.0), ``nonzero`` counts like ``np.count_nonzero`` (NaNs
    included).  ``t`` as in ``device_order_statistics`` (read once here).  One host synchronisation."""
    return _read_extremes(_launch_extremes(t, "device_extremes"))


class _HostChunks:
    """A host array as device pieces of at most ``chunk_elems`` elements, uploaded anew on every iteration."""

    def __init__(self, arr: np.ndarray, chunk_elems: int, device):
        self.flat, self.step, self.device = np.ascontiguousarray(arr).reshape(-1), max(int(chunk_elems), 1), device

    def __iter__(self):
        for off in range(0, self.flat.size, self.step):
            yield torch.from_numpy(self.flat[off:off + self.step]).to(self.device)


class DeviceNPZDataset(NPZSequenceDataset):
    """``NPZSequenceDataset`` whose normalisation constants come from the device: the same constructor arguments, attributes,
    ``__getitem__`` and ``denormalize``, and the same values bit for bit, but ``np.max(X)`` is one ``uclstm_dataset_extremes``
    pass and every percentile the host constructor would take comes out of ONE radix select over ``Y`` (up to 6 order
    statistics, three passes), launched only on the branches the host constructor takes.  The percentiles of the TRANSFORMED
    targets need no pass of their own: the transforms are monotone, so they are the transform of the same two order statistics
    of the raw ``Y``, finished on the host with numpy's own ``arcsinh`` / ``log1p`` and numpy's f32 rank rule
    (``percentile_ranks``; above 2^24 elements that rule rounds the rank itself, which is kept for parity).

    When ``X`` and ``Y`` fit ``max_resident_bytes`` (default: 80 % of the device memory free at that moment) they are uploaded
    once and left in the cache that ``DeviceSequenceLoader`` reads, so a loader over this dataset uploads nothing.  Otherwise
    they are streamed in pieces of ``chunk_bytes``, once per pass, and the cache stays empty (``DeviceSequenceLoader`` then raises
    its "does not fit" error as before)."""

    def __init__(self, npz_path, lower_percentile=0.00001, upper_percentile=99.99999, clip_outliers=True,
                 min_y=-7.5987958908081055, max_y=8.784920692443848, y_transform="asinh", y_transform_scale=None,
                 y_transform_percentile=99, device="cuda", max_resident_bytes: Optional[int] = None, chunk_bytes: int = 256 << 20):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.L.UclstmError(f"DeviceNPZDataset: a HIP device is required, got {dev} (this package has no CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        if int(chunk_bytes) < 4:
            raise ValueError(f"DeviceNPZDataset: chunk_bytes must hold at least one element, got {chunk_bytes}")
        if y_transform not in ("asinh", "signed_log", None, "none"):
            raise ValueError(y_transform)
        with np.load(npz_path, allow_pickle=False) as data:
            self.X = data["X"].astype(np.float32)
            self.Y = data["Y"].astype(np.float32)
        self.N, self.T, _, self.H, self.W = self.X.shape
        if self.Y.ndim == 5 and self.Y.shape[2] > 1:
            raise TypeError(f"DeviceNPZDataset does not take a vector dataset: Y has {self.Y.shape[2]} target channels and this class "
                            "derives one scalar set of constants; VectorNPZDataset computes per-channel constants on the host")
        need = int(self.X.nbytes) + int(self.Y.nbytes)
        limit = int(0.8 * torch.cuda.mem_get_info(dev)[0]) if max_resident_bytes is None else int(max_resident_bytes)
        if need <= limit:
            self._device_resident = {dev: (torch.from_numpy(np.ascontiguousarray(self.X)).to(dev),
                                           torch.from_numpy(np.ascontiguousarray(self.Y)).to(dev))}
            x_src, y_src = self._device_resident[dev]
        else:
            x_src, y_src = _HostChunks(self.X, int(chunk_bytes) // 4, dev), _HostChunks(self.Y, int(chunk_bytes) // 4, dev)
        self.y_transform, self.clip_outliers = y_transform, clip_outliers
        explicit = (min_y is not None) and (max_y is not None)
        # the order statistics the host constructor's branches read, all in one select
        n = int(self.Y.size)
        want = {}                       # name -> (q, kind) of the percentiles this call takes
        if y_transform_scale is None and y_transform_percentile is not None:
            want["scale"] = (y_transform_percentile, "abs")
        if not explicit:
            want["lo"], want["hi"] = (lower_percentile, "signed"), (upper_percentile, "signed")
        rk = {name: percentile_ranks(n, q) for name, (q, _) in want.items()}
        x_out = _launch_extremes(x_src, "DeviceNPZDataset X")
        sel = _launch_select(y_src, [r for name in want for r in rk[name][:2]], [want[name][1] for name in want for _ in range(2)],
                             "DeviceNPZDataset Y") if want else None
        xs = _read_extremes(x_out)
        self.x_max = float("nan") if xs["nan_count"] else xs["max"]
        self.norm_const = max(self.x_max, 1.0)
        values, nan = (None, 0) if sel is None else _read_select(sel, 2 * len(want))[:2]
        pair = {name: values[2 * i:2 * i + 2] for i, name in enumerate(want)}

        def pct(name, fwd=None):
            """numpy's percentile from its two order statistics; ``fwd``: that of the transformed array (monotone: same ranks)."""
            if nan:
                return float("nan")
            a, b = pair[name] if fwd is None else fwd(pair[name])
            return float(percentile_lerp(a, b, rk[name][2]))
        if y_transform_scale is None:
            self.y_scale = pct("scale") if y_transform_percentile is not None else 1.0
        else:
            self.y_scale = float(y_transform_scale)
        if explicit:
            self.min_vel, self.max_vel = float(min_y), float(max_y)
            self.trans_min = float(self._fwd(np.float64(self.min_vel)))
            self.trans_max = float(self._fwd(np.float64(self.max_vel)))
        else:
            self.min_vel, self.max_vel = pct("lo"), pct("hi")
            self.trans_min, self.trans_max = pct("lo", self._fwd), pct("hi", self._fwd)
            if self.y_scale == 0.0 and self.y_transform in ("asinh", "signed_log"):
                # the one case where the transformed ARRAY holds NaNs that its two order statistics do not show: 0 / 0 at every
                # zero target.  numpy's percentile of it is NaN then; one extremes pass tells whether there is such a target.
                ys = device_extremes(y_src)
                if ys["nonzero"] < ys["count"]:
                    self.trans_min = self.trans_max = float("nan")
        if self.trans_max == self.trans_min:
            self.trans_max = self.trans_min + 1.0


# ---------------------------------------------------------------------------------------------
# moving sprites (Moving-MNIST, digits/build_moving_mnist.py) rendered on the device
# ---------------------------------------------------------------------------------------------
MAX_SPRITES, MAX_GLYPH, MAX_SPRITE_SPEED = 8, 64, 127          # what uclstm_sprites_render accepts / clamps to


def _glyph_bank(bank) -> np.ndarray:
    """``bank`` (numpy array or CPU tensor) as a contiguous uint8 ``[n_glyph, gh, gw]`` array; ``ValueError`` otherwise."""
    b = bank.detach().cpu().numpy() if isinstance(bank, torch.Tensor) else np.asarray(bank)
    if b.dtype != np.uint8 or b.ndim != 3 or min(b.shape) < 1:
        raise ValueError(f"glyph bank: expected uint8 [n_glyph, gh, gw], got {b.dtype} {tuple(b.shape)}")
    if max(b.shape[1:]) > MAX_GLYPH:
        raise ValueError(f"glyph bank: glyphs of {b.shape[1]} x {b.shape[2]} exceed {MAX_GLYPH} x {MAX_GLYPH}")
    return np.ascontiguousarray(b)


def load_idx_images(path) -> np.ndarray:
    """An MNIST IDX image file the user already has (``train-images-idx3-ubyte``, plain or ``.gz``) as uint8
    ``[n, rows, cols]``: big-endian header {magic 2051, n, rows, cols}, then the bytes.  Nothing is ever downloaded."""
    import gzip
    path = str(path)
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        head = f.read(16)
        if len(head) != 16:
            raise ValueError(f"{path}: not an IDX image file (header of {len(head)} bytes)")
        magic, n, rows, cols = (int(v) for v in np.frombuffer(head, dtype=">u4"))
        if magic != 2051:
            raise ValueError(f"{path}: not an IDX image file (magic {magic}, expected 2051)")
        data = f.read(n * rows * cols + 1)
    if len(data) != n * rows * cols:
        raise ValueError(f"{path}: header says {n} images of {rows} x {cols}, the file holds "
                         f"{'more' if len(data) > n * rows * cols else len(data)} bytes")
    return np.frombuffer(data, dtype=np.uint8).reshape(n, rows, cols).copy()


def procedural_glyphs(n: int, size: int = 28, seed: int = 0) -> np.ndarray:
    """A built-in glyph bank, uint8 ``[n, size, size]``: per glyph three soft strokes (bumps ``1 / (1 + q)^2`` along line
    segments) inside a margin of background, quantised to bytes with everything below 0.2 cut to 0.  IEEE basic operations
    (+, -, *, /, min, max, floor) in f64 only and ``torch.rand`` of a seeded CPU generator for the stroke ends, so the bank is
    identical on every host (``exp()`` and friends differ by an ulp between vector ISAs).  Tests and tools use it in place of
    MNIST digits."""
    n, size = int(n), int(size)
    if n < 1 or not 8 <= size <= MAX_GLYPH:
        raise ValueError(f"procedural_glyphs: n >= 1 and 8 <= size <= {MAX_GLYPH} are required, got n {n}, size {size}")
    ends = torch.rand((n, 3, 4), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64).numpy()
    lo, span = 0.18 * size, 0.64 * size
    ends = lo + span * ends                                              # [n, stroke, (ax, ay, bx, by)] in pixels
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    width = 0.045 * size + 0.4
    img = np.zeros((n, size, size), dtype=np.float64)
    for s in range(3):
        ax, ay, bx, by = (ends[:, s, i][:, None, None] for i in range(4))
        ex, ey = bx - ax, by - ay
        u = ((xx - ax) * ex + (yy - ay) * ey) / (ex * ex + ey * ey + 1e-9)
        u = np.minimum(np.maximum(u, 0.0), 1.0)                          # the nearest point of the segment
        dx, dy = xx - (ax + u * ex), yy - (ay + u * ey)
        q = (dx * dx + dy * dy) / (2.0 * width * width)
        img = np.maximum(img, 1.0 / ((1.0 + q) * (1.0 + q)))
    img = np.where(img < 0.2, 0.0, img)
    return np.floor(img * 255.0 + 0.5).astype(np.uint8)


def check_sprite_table(table, n_glyph: int, H: int, W: int, gh: int, gw: int, max_speed: int = MAX_SPRITE_SPEED) -> np.ndarray:
    """Validate a sprite table (integer ``[n, D, 5]`` rows ``{glyph, x0, y0, vx, vy}``) before anything is uploaded and return
    it as a contiguous int32 array.  ``ValueError`` for a wrong shape or dtype, ``D`` outside 1..8, a glyph outside
    ``[0, n_glyph)``, ``x0`` outside ``[0, W - gw]``, ``y0`` outside ``[0, H - gh]`` or a speed above ``max_speed`` (at most
    127, the kernel's own clamp).  The kernel clamps the same quantities, so a bad table is never a wild access -- this
    function is what refuses it."""
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.dtype.kind not in "iu" or t.ndim != 3 or t.shape[2] != 5:
        raise ValueError(f"sprite table: expected integers [n, D, 5], got {t.dtype} {tuple(t.shape)}")
    if not 1 <= t.shape[1] <= MAX_SPRITES:
        raise ValueError(f"sprite table: D must be in 1..{MAX_SPRITES}, got {t.shape[1]}")
    if gw > W or gh > H or not 0 <= int(max_speed) <= MAX_SPRITE_SPEED:
        raise ValueError(f"sprite table: glyphs of {gh} x {gw} must fit the {H} x {W} frame and max_speed be in "
                         f"0..{MAX_SPRITE_SPEED}, got {max_speed}")
    t64 = t.astype(np.int64)
    for col, name, lo, hi in ((0, "glyph", 0, int(n_glyph) - 1), (1, "x0", 0, W - gw), (2, "y0", 0, H - gh),
                              (3, "vx", -int(max_speed), int(max_speed)), (4, "vy", -int(max_speed), int(max_speed))):
        bad = (t64[..., col] < lo) | (t64[..., col] > hi)
        if bad.any():
            i, d = (int(v[0]) for v in np.nonzero(bad))
            raise ValueError(f"sprite table: {name} = {int(t64[i, d, col])} of sequence {i}, sprite {d} is outside [{lo}, {hi}]")
    return np.ascontiguousarray(t64.astype(np.int32))


def epoch_sprites(n: int, D: int, n_glyph: int, H: int, W: int, gh: int, gw: int, max_speed: int = 5, generator=None) -> np.ndarray:
    """The sprite table of one epoch: int32 ``[n, D, 5]`` rows ``{glyph, x0, y0, vx, vy}`` -- a pure function of its arguments
    and the generator's state.  Drawn with ``torch.randint(..., (n, D), generator=generator)`` on the CPU in this order: all
    glyph indices (uniform over ``[0, n_glyph)``), then all ``x0`` (uniform over ``[0, W - gw]``), then all ``y0``
    (``[0, H - gh]``), then all ``vx``, then all ``vy`` (uniform integers in ``[-max_speed, max_speed]``; the reference uses
    5, build_moving_mnist.py:17-21).  A column with a single possible value (``W == gw``, one glyph, ``max_speed == 0``) is
    that value and draws nothing.  So a seeded generator reproduces an epoch, and the next call continues the stream."""
    n, D, max_speed = int(n), int(D), int(max_speed)
    if not 1 <= D <= MAX_SPRITES or n_glyph < 1 or gw > W or gh > H or min(gh, gw) < 1 or not 0 <= max_speed <= MAX_SPRITE_SPEED:
        raise ValueError(f"epoch_sprites: D in 1..{MAX_SPRITES}, n_glyph >= 1, glyphs that fit the frame and max_speed in "
                         f"0..{MAX_SPRITE_SPEED} are required, got D {D}, n_glyph {n_glyph}, {gh} x {gw} in {H} x {W}, speed {max_speed}")
    tab = np.zeros((max(n, 0), D, 5), dtype=np.int32)
    if n <= 0:
        return tab
    for col, lo, count in ((0, 0, int(n_glyph)), (1, 0, W - gw + 1), (2, 0, H - gh + 1), (3, -max_speed, 2 * max_speed + 1),
                           (4, -max_speed, 2 * max_speed + 1)):
        if count > 1:
            tab[:, :, col] = torch.randint(0, count, (n, D), generator=generator).numpy().astype(np.int32) + lo
    return tab


def render_sprites_host(bank, table, T: int, H: int, W: int) -> np.ndarray:
    """Host mirror of ``uclstm_sprites_render`` in numpy: f32 ``[n, T, 2, H, W]``, channel 0 the frame and channel 1 the raw
    velocity map -- the ``data`` array of the reference's ``generate_moving_mnist`` (digits/build_moving_mnist.py:5-58) for the
    draws recorded in ``table``, for any frame and glyph size.  Per sequence, sprites in table order, frames in time order:
    where the glyph byte is non-zero the frame takes ``byte / 255`` (a later sprite overwrites) and the map adds the sprite's
    current ``vx``; then the sprite moves, and a position outside ``[0, W - gw]`` / ``[0, H - gh]`` flips that velocity
    component and is clamped.  Vectorised over sequences and glyph pixels; the table is validated first."""
    bank = _glyph_bank(bank)
    K, gh, gw = bank.shape
    tab = check_sprite_table(table, K, H, W, gh, gw).astype(np.int64)
    n, D = tab.shape[:2]
    out = np.zeros((n, int(T), 2, H, W), dtype=np.float32)
    level = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)       # build_moving_mnist.py:26, stored as f32 (:10)
    for d in range(D):
        glyph = bank[tab[:, d, 0]]                                               # [n, gh, gw]
        ni, ri, ci = np.nonzero(glyph)                                           # the covered pixels, the same in every frame
        value = level[glyph[ni, ri, ci]]
        px, py, vx, vy = (tab[:, d, c].copy() for c in (1, 2, 3, 4))
        for t in range(int(T)):
            out[ni, t, 0, py[ni] + ri, px[ni] + ci] = value
            out[ni, t, 1, py[ni] + ri, px[ni] + ci] += vx[ni].astype(np.float32)
            px, py = px + vx, py + vy
            hit = (px < 0) | (px > W - gw)
            vx = np.where(hit, -vx, vx)
            px = np.clip(px, 0, W - gw)
            hit = (py < 0) | (py > H - gh)
            vy = np.where(hit, -vy, vy)
            py = np.clip(py, 0, H - gh)
    return out


def _render_sprites(bank, table, n_out, shape, v_scale, out=None, raw=None):
    """One launch of ``uclstm_sprites_render``: device ``bank`` (uint8 ``[n_glyph, gh, gw]``) and ``table`` (int32
    ``[>= n_out, D, 5]``) -> ``(x [n_out,T,C,H,W], y, mask [n_out,T,1,H,W])``; ``shape = (T, C, H, W)``.  ``out``: caller-owned
    ``(x, y, mask)`` to write into, fresh tensors on the current stream otherwise; ``raw``: an optional ``[n_out,T,2,H,W]``
    buffer for the reference's ``data`` layout.  Nothing is pre-zeroed: the kernel writes every element."""
    from . import _lib as L
    T, Cc, H, W = (int(v) for v in shape)
    if not (isinstance(bank, torch.Tensor) and bank.is_cuda and bank.dtype == torch.uint8 and bank.dim() == 3 and bank.is_contiguous()):
        raise L.UclstmError("_render_sprites: bank must be a contiguous uint8 [n_glyph, gh, gw] HIP device tensor")
    table = ops._dev(table, torch.int32, "sprite table")
    if table.dim() != 3 or table.shape[2] != 5 or table.shape[0] < n_out or table.device != bank.device:
        raise L.UclstmError(f"_render_sprites: table must be int32 [>= {n_out}, D, 5] on {bank.device}, got {tuple(table.shape)}")
    if out is None:
        x = torch.empty((n_out, T, Cc, H, W), dtype=torch.float32, device=bank.device)
        y = torch.empty((n_out, T, 1, H, W), dtype=torch.float32, device=bank.device)
        mask = torch.empty_like(y)
    else:
        x, y, mask = out
    for t, want, what in ((x, (n_out, T, Cc, H, W), "x"), (y, (n_out, T, 1, H, W), "y"), (mask, (n_out, T, 1, H, W), "mask"),
                          (raw, (n_out, T, 2, H, W), "raw")):
        if t is None and what == "raw":
            continue
        ops._dev(t, torch.float32, what)
        if tuple(t.shape) != want or t.device != bank.device:
            raise L.UclstmError(f"_render_sprites: {what} must be {want} on {bank.device}, got {tuple(t.shape)} on {t.device}")
    L.check(L.lib.uclstm_sprites_render(ops._p(bank), bank.shape[0], bank.shape[1], bank.shape[2], ops._p(table), n_out,
                                        table.shape[1], T, Cc, H, W, float(v_scale), ops._p(x), ops._p(y), ops._p(mask),
                                        ops._p(raw), ops._stream()), "sprites_render")
    return x, y, mask


class DeviceSpriteLoader:
    """An endless Moving-MNIST source (digits/build_moving_mnist.py) that behaves like a ``DataLoader``: every batch is
    RENDERED on the GPU by one launch of ``uclstm_sprites_render`` -- no file, no host arithmetic, no host-to-device copy of
    pixels.  Yields ``(x [b,T,C,H,W], y [b,T,1,H,W], mask [b,T,1,H,W])`` as fresh f32 device tensors on the current stream:
    ``x`` is the frame in every channel (both "satellite" views see the same scene, as ``SyntheticSequences(kind="blobs")``
    has it), ``y`` the per-pixel map of summed horizontal velocities over ``v_scale``, ``mask`` the sprite pixels.

    ``bank``: uint8 ``[n_glyph, gh, gw]`` glyphs (``load_idx_images`` of an MNIST file, ``procedural_glyphs``), uploaded once.
    ``len()`` is ``steps_per_epoch``.  Each epoch draws ONE table for ``steps_per_epoch * batch_size`` sequences with
    ``epoch_sprites(..., generator)``, validates it (``check_sprite_table``) and uploads it as one pinned int32 tensor;
    ``last_table`` keeps the host copy, and ``render_sprites_host(bank, last_table, T, H, W)`` is the epoch bit for bit.  Per
    batch nothing is copied and nothing synchronises.  ``fixed=True`` draws the table once at construction: every epoch is
    then the same set -- a validation set.

    It also stands in for the ``dataset_obj`` of ``train_one_epoch`` / ``evaluate`` / ``EvalReport``: ``y_transform = None``,
    ``y_scale = 1.0``, ``trans_min = -v_scale``, ``trans_max = +v_scale`` and ``denormalize(y) = y * v_scale`` (pixels per
    frame), so ``train_one_epoch(model, loader, opt, dev, loader)`` runs unchanged.

    Under ``FlatDDP`` every rank constructs its own loader and passes its OWN seeded generator (for instance
    ``torch.Generator().manual_seed(seed + rank)``): ranks that share a seed would render the same sequences."""

    y_transform = None
    y_scale = 1.0

    def __init__(self, bank, batch_size: int, steps_per_epoch: int, T: int = 20, H: int = 64, W: int = 64, num_sprites: int = 2,
                 max_speed: int = 5, channels: int = 2, v_scale: float = 5.0, generator=None, fixed: bool = False, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.L.UclstmError(f"DeviceSpriteLoader: a HIP device is required, got {dev} (this package has no CPU path)")
        host = _glyph_bank(bank)
        self.batch_size, self.steps_per_epoch = int(batch_size), int(steps_per_epoch)
        self.T, self.H, self.W, self.channels = int(T), int(H), int(W), int(channels)
        self.num_sprites, self.max_speed, self.v_scale = int(num_sprites), int(max_speed), float(v_scale)
        if self.batch_size <= 0 or self.steps_per_epoch <= 0 or self.T < 1 or self.channels < 1 or not self.v_scale > 0.0:
            raise ValueError("DeviceSpriteLoader: batch_size, steps_per_epoch, T, channels and v_scale must be positive")
        epoch_sprites(0, self.num_sprites, host.shape[0], self.H, self.W, host.shape[1], host.shape[2], self.max_speed)   # validates
        self.trans_min, self.trans_max = -self.v_scale, self.v_scale
        self.generator, self.fixed, self.last_table = generator, bool(fixed), None
        self.device = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        self.bank_host = host
        self.bank = torch.from_numpy(host).to(self.device)
        self._fixed = self._draw() if self.fixed else None

    def _draw(self):
        """Draw, validate and upload one epoch's table: (pinned host tensor, device tensor)."""
        K, gh, gw = self.bank_host.shape
        tab = epoch_sprites(self.steps_per_epoch * self.batch_size, self.num_sprites, K, self.H, self.W, gh, gw, self.max_speed,
                            self.generator)
        self.last_table = check_sprite_table(tab, K, self.H, self.W, gh, gw, self.max_speed)
        pinned = torch.from_numpy(self.last_table).pin_memory()
        return pinned, pinned.to(self.device, non_blocking=True)

    def denormalize(self, y_norm):
        """``y * v_scale``: summed horizontal velocity in pixels per frame (numpy or torch, any device)."""
        return y_norm * self.v_scale

    def __len__(self):
        return self.steps_per_epoch

    def __iter__(self):
        return self.batches()

    def batches(self, out=None):
        """The epoch's batches.  ``out=(x, y, mask)``: every batch is rendered into these caller-owned contiguous f32 device
        buffers, which are yielded themselves -- the static inputs of a ``GraphedTrainStep``."""
        b, shape = self.batch_size, (self.T, self.channels, self.H, self.W)
        if out is not None:
            want = ((b, self.T, self.channels, self.H, self.W), (b, self.T, 1, self.H, self.W), (b, self.T, 1, self.H, self.W))
            if len(out) != 3:
                raise ValueError("batches(out=...): expected (x, y, mask)")
            for t, w, what in zip(out, want, ("out x", "out y", "out mask")):
                ops._dev(t, torch.float32, what)
                if tuple(t.shape) != w or t.device != self.device:
                    raise ValueError(f"batches(out=...): {what} must be {w} on {self.device}, got {tuple(t.shape)} on {t.device}")
        return self._run(out, b, shape)

    def _run(self, out, b, shape):
        # ONE pinned int32 tensor per epoch, copied without blocking; this generator's frame keeps it alive until the epoch ends
        pinned, table = self._fixed if self.fixed else self._draw()
        for s in range(self.steps_per_epoch):
            yield _render_sprites(self.bank, table[s * b:(s + 1) * b], b, shape, self.v_scale, out)
        del pinned


# ---------------------------------------------------------------------------------------------
# step / epoch loops
# ---------------------------------------------------------------------------------------------
def _stack(output):
    pre = getattr(output, "stacked", None)          # modules.SeqList: the frames as one [B,T,...] view of the kernel's output
    if pre is not None:
        return pre
    return torch.stack(output, dim=1) if isinstance(output, (list, tuple)) else output      # main.py:97-100


def train_step(model, optimizer, x, y, mask=None, use_mask=True, ddp=None, clip_norm: Optional[float] = 1.0,
               loss: Optional[LossSpec] = None):
    """zero_grad -> forward -> stack -> loss -> backward -> [gradient all-reduce] -> clip(1.0) -> optimiser step
    (main.py:91-108).  Returns ``(loss, y_pred)`` as device tensors; nothing here waits for the GPU.  ``loss``: the
    ``LossSpec`` of ``compute_loss(spec=...)``; None is the reference's loss."""
    spec = check_spec(loss)
    if getattr(getattr(optimizer, "ema", None), "_swapped", False):      # optimizer.step() would refuse: do so before BatchNorm's buffers move
        raise RuntimeError("train_step inside WeightEMA.swapped(): the parameters hold the averaged weights there")
    optimizer.zero_grad(set_to_none=True)
    if ddp is not None:
        ddp.reset()
    on_gpu = x.is_cuda
    if on_gpu:
        from . import ops
        ops.prepack_begin()          # weights are fixed until optimizer.step(): pack this step's panels ahead, off the main stream
    # FlatDDP(sync_bn=True): forward and backward run with BatchNorm statistics over the wrapper's process group
    sync = contextlib.nullcontext()
    if ddp is not None and getattr(ddp, "sync_bn", False) and on_gpu:
        sync = ops.sync_batchnorm(ddp.pg)
    try:
        with sync:
            output, _ = model(x)
            y_pred = _stack(output)
            loss = compute_loss(y_pred, y, mask, use_mask, spec)
            # fp16 compute: backward runs on loss * scale (FusedAdamW(loss_scale=...) owns the device-side dynamic scale)
            (optimizer.scale_loss(loss) if hasattr(optimizer, "scale_loss") else loss).backward()
    finally:
        if on_gpu:
            ops.prepack_end()
    if ddp is not None:
        ddp.finalize()
    if isinstance(optimizer, FusedAdamW):
        optimizer.max_grad_norm = clip_norm          # clip fused into the optimiser kernels (device-side coefficient)
    elif clip_norm is not None:
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip_norm)                         # main.py:106
    optimizer.step()
    return loss.detach(), y_pred.detach()


class GraphedTrainStep:
    """``train_step`` captured ONCE as a HIP graph and replayed: a training step is ~400 kernel launches issued from Python
    through ctypes (12-19 ms of host time); at the per-GPU batch the benchmark uses the device needs longer than that, but at
    small batches (strong scaling: a global batch of 32 over 8 GPUs is 4 sequences each) the step is bound by the host.  A
    replay costs the host one call.

    What makes the step capturable: no host synchronisation anywhere in it; the optimiser reads its hyper-parameters and step
    count from device memory (``FusedAdamW(capturable=True)``); the weight-gradient / BatchNorm side stream forks from and joins
    the capturing stream through events; the look-ahead panel packing uses a persistent job table.  Inputs are copied into
    static buffers; ``loss`` / ``y_pred`` are static outputs (valid until the next call).  Shapes, ``use_mask``, the ``loss``
    keyword (a ``LossSpec`` or None, kept as ``self.loss_spec``) and the model's mode are fixed at capture; ``clip_norm`` / lr changes (of every parameter group) reach the device through
    ``optimizer.sync_hyper()`` before a replay.  fp16 compute (``ops.compute_dtype(torch.float16)`` around construction and
    calls, ``FusedAdamW(loss_scale=..., capturable=True)``): the loss scale, the overflow test, the skipped step and the scale
    update all live on the device, so an overflowed replay leaves parameters and moments alone without the host knowing.
    Data-parallel training keeps the eager step (its collectives are launched from backward hooks).

    Deterministic mode (``ops.deterministic()`` / ``ops.set_deterministic``) is part of what is captured: the graph holds the
    ordered or the atomic reductions according to the switch at construction (``self.deterministic``), and every replay keeps
    that mode whatever the switch says later."""

    def __init__(self, model, optimizer, x, y, mask=None, use_mask: bool = True, clip_norm: Optional[float] = 1.0, warmup: int = 3,
                 loss: Optional[LossSpec] = None):
        self.loss_spec = check_spec(loss)
        if not (isinstance(optimizer, FusedAdamW) and optimizer.capturable):
            raise ValueError("GraphedTrainStep needs FusedAdamW(..., capturable=True)")
        if not x.is_cuda:
            raise ops.L.UclstmError("GraphedTrainStep: HIP device tensors required")
        if ops.get_sync_batchnorm() is not None:
            raise ops.L.UclstmError("GraphedTrainStep: sync_batchnorm is on -- the step then contains collectives, and a graphed "
                                    "step is single-rank only; turn the switch off or use the eager train_step")
        self.model, self.optimizer, self.use_mask, self.clip_norm = model, optimizer, use_mask, clip_norm
        self.deterministic = ops.is_deterministic()
        self.x, self.y = x.clone(), y.clone()
        self.mask = None if mask is None else mask.clone()
        optimizer.max_grad_norm = clip_norm
        optimizer.sync_hyper()
        # eager warm-up steps on a side stream (the capture runs on one too): the look-ahead packing plan, the stream pair,
        # the caching allocator's pools and every first-launch attribute call exist before the capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(max(warmup, 2)):
                train_step(model, optimizer, self.x, self.y, self.mask, use_mask, None, clip_norm, self.loss_spec)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.y_pred = train_step(model, optimizer, self.x, self.y, self.mask, use_mask, None, clip_norm, self.loss_spec)
        # The graph owns what it captured.  Everything the capture allocated lives in the graph's own pool, and the model, the
        # optimiser and the static inputs are held above; the look-ahead batch is the exception: its panels and its device job
        # table were allocated by an eager step BEFORE the capture, their addresses are baked into the graph, and their only
        # other owner is the module global ops._PACK_BATCH, which prepack_begin() replaces as soon as another plan comes along
        # (an eager step of a second model, or of this one after a freeze).  Without this reference a later replay would read
        # a freed job table and write freed panels.
        self._pack_batch = ops._PACK_BATCH if (ops.PREPACK and ops.PACK_BATCHED) else None
        if ops.PREPACK and ops.PACK_BATCHED and self._pack_batch is None:
            raise ops.L.UclstmError("GraphedTrainStep: look-ahead packing is on but the capture used no batch (no pack call in the step?)")
        # likewise the plane-weight table of a WeightedLossSpec: built by the first warm-up step, its address is in the graph
        self._plane_w = ops.plane_weight_table(self.loss_spec, self.y_pred)[0] if getattr(self.loss_spec, "weighted", False) else None
        self.replays = 0

    def __call__(self, x, y, mask=None):
        if x is not self.x:
            self.x.copy_(x, non_blocking=True)
        if y is not self.y:
            self.y.copy_(y, non_blocking=True)
        if self.mask is not None and mask is not None and mask is not self.mask:
            self.mask.copy_(mask, non_blocking=True)
        self.optimizer.max_grad_norm = self.clip_norm
        self.optimizer.sync_hyper()
        if self.optimizer.ema is not None and self.optimizer.ema._swapped:          # what optimizer.step() refuses in an eager step
            raise RuntimeError("GraphedTrainStep inside WeightEMA.swapped(): the parameters hold the averaged weights there")
        self.graph.replay()
        self.replays += 1
        ops.weights_changed()          # what optimizer.step() tells the panel caches in an eager step
        return self.loss, self.y_pred


class _Metrics:
    """Running sums of |d|, d^2, d and the count on the device (replaces main.py:114-142)."""

    def __init__(self, device):
        self.s = torch.zeros(4, dtype=torch.float64, device=device)
        self.sv = None                               # [Cy, 4] for a vector dataset: the same sums per target channel

    @torch.no_grad()
    def _add_vec(self, ds, y, y_pred, mask, use_mask):
        """One ``uclstm_metric_sums_vec`` (ordered partials in both modes): every channel de-normalised with its own constants."""
        from . import _lib as L
        yp = ops._dev(y_pred.contiguous().float(), torch.float32, "y_pred")
        yt = ops._dev(y.contiguous().float(), torch.float32, "y")
        Cy, (H, W) = ds.Cy, yp.shape[-2:]
        if yp.dim() < 3 or yp.shape[-3] != Cy or yt.shape != yp.shape:
            raise ValueError(f"metrics: y_pred and y must be [..., {Cy}, H, W], got {tuple(yp.shape)} and {tuple(yt.shape)}")
        n_frames = yp.numel() // (Cy * H * W)
        m = None
        if use_mask and mask is not None:
            m = ops._dev(mask.contiguous().float(), torch.float32, "mask")
            if m.numel() != n_frames * H * W:
                raise ValueError(f"metrics: the mask of a vector target has one channel, [..., 1, {H}, {W}]; got {tuple(m.shape)}")
        if self.sv is None:
            self.sv = torch.zeros((Cy, 4), dtype=torch.float64, device=yp.device)
        partials = torch.empty((int(L.lib.uclstm_metric_sums_vec_rows(n_frames, Cy, H * W)), Cy, 4), dtype=torch.float64, device=yp.device)
        ops._log_reduce("metric_sums_vec")
        L.check(L.lib.uclstm_metric_sums_vec(ops._p(yp), ops._p(yt), ops._p(m), ops._p(partials), ops._p(self.sv), 1, n_frames, Cy, H * W,
                                             _TRANSFORM_IDS[ds.y_transform], ds.target_consts(), ops._stream()), "metric_sums_vec")

    @torch.no_grad()
    def add(self, dataset_obj, y, y_pred, mask, use_mask):
        if isinstance(dataset_obj, VectorNPZDataset):
            return self._add_vec(dataset_obj, y, y_pred, mask, use_mask)
        if y_pred.is_cuda and getattr(dataset_obj, "y_transform", None) == "asinh" and hasattr(dataset_obj, "trans_min"):
            # one fused kernel: de-normalise both, difference, masked running sums (no intermediate tensors)
            from . import _lib as L
            yp = y_pred.contiguous().float()
            yt = y.contiguous().float()
            m = mask.contiguous().float() if (use_mask and mask is not None) else None
            if ops.is_deterministic():
                partials = torch.empty((int(L.lib.uclstm_metric_sums_ordered_rows(yp.numel())), 4), dtype=torch.float64, device=yp.device)
                ops._log_reduce("metric_sums_ordered")
                L.check(L.lib.uclstm_metric_sums_ordered(ops._p(yp), ops._p(yt), ops._p(m), ops._p(partials), ops._p(self.s), 1, yp.numel(),
                                                         float(dataset_obj.y_scale), float(dataset_obj.trans_min),
                                                         float(dataset_obj.trans_max), ops._stream()), "metric_sums_ordered")
                return
            ops._log_reduce("metric_sums")
            L.check(L.lib.uclstm_metric_sums(ops._p(yp), ops._p(yt), ops._p(m), ops._p(self.s), yp.numel(),
                                             float(dataset_obj.y_scale), float(dataset_obj.trans_min), float(dataset_obj.trans_max),
                                             ops._stream()), "metric_sums")
            return
        d = (dataset_obj.denormalize(y_pred) - dataset_obj.denormalize(y)).double()
        if use_mask:
            m = (mask != 0).double()
            self.s += torch.stack(((d.abs() * m).sum(), (d * d * m).sum(), (d * m).sum(), m.sum()))
        else:
            self.s += torch.stack((d.abs().sum(), (d * d).sum(), d.sum(),
                                   torch.tensor(float(d.numel()), dtype=torch.float64, device=d.device)))

    def result(self):
        """``(mae, rmse, me)``; for a vector dataset pooled over the channels (the sums of all channels added in channel order)."""
        a, q, e, n = (float(v) for v in (self.s if self.sv is None else self.sv.sum(dim=0)).cpu())
        if n <= 0:
            return 0.0, 0.0, 0.0
        return a / n, math.sqrt(q / n), e / n

    def per_channel(self):
        """``{"mae": [Cy], "rmse": [Cy], "me": [Cy]}``; a scalar dataset is one channel."""
        rows = (self.s.reshape(1, 4) if self.sv is None else self.sv).cpu().tolist()
        out = {"mae": [], "rmse": [], "me": []}
        for a, q, e, n in rows:
            out["mae"].append(a / n if n > 0 else 0.0)
            out["rmse"].append(math.sqrt(q / n) if n > 0 else 0.0)
            out["me"].append(e / n if n > 0 else 0.0)
        return out


def quiesce_host_gc() -> None:
    """Collect once and move every object alive now into the permanent generation (``gc.freeze``).

    A training step is ~500 kernel launches from Python; the host runs 1-3 steps ahead of the device.  A full (generation 2)
    garbage collection of a process that has imported torch walks ~10^6 objects and stops the host for ~75 ms (measured,
    ``tools/spike_hunt.py``): whenever the host is less than that ahead -- after any synchronisation: the start of an epoch,
    a ``loss.item()``, a benchmark's timed region -- the device runs dry and ONE step takes 60-130 ms instead of 33.  After
    ``gc.freeze()`` later collections only walk objects created since, which takes microseconds.  Call it once the model,
    the optimiser and the first steps' caches exist; ``train_one_epoch`` does after its second step.
    """
    import gc
    gc.collect()
    gc.freeze()


def train_one_epoch(model, loader, optimizer, device, dataset_obj, use_mask=True, per_channel: bool = False, ddp=None,
                    loss: Optional[LossSpec] = None):
    """Reference main.py:77-144; returns ``(avg_loss, avg_mae, avg_rmse, avg_me)``.  ``loss``: as in ``train_step``.
    For a ``VectorNPZDataset`` the three metrics are pooled over the target channels; ``per_channel=True`` appends
    ``{"mae": [Cy], "rmse": [Cy], "me": [Cy]}``."""
    spec = check_spec(loss)
    model.train()
    total = torch.zeros((), dtype=torch.float64, device=device)
    n = 0
    met = _Metrics(device)
    for it, (x, y, mask) in enumerate(loader):
        if it == 2:
            quiesce_host_gc()
        x, y, mask = x.to(device, non_blocking=True), y.to(device, non_blocking=True), mask.to(device, non_blocking=True)
        loss, y_pred = train_step(model, optimizer, x, y, mask, use_mask, ddp, loss=spec)
        total += loss.double() * x.size(0)
        n += x.size(0)
        met.add(dataset_obj, y, y_pred, mask, use_mask)
    mae, rmse, me = met.result()
    return (float(total) / max(n, 1), mae, rmse, me) + ((met.per_channel(),) if per_channel else ())


@torch.no_grad()
def _evaluate(model, loader, device, dataset_obj, use_mask, tta, spec, report=None):
    """The loop of ``evaluate``, ``evaluate_report`` and ``evaluate_vector_report``: ``(avg_loss, _Metrics)``; every batch's
    ``y_pred`` also goes to ``report.add`` when there is a report."""
    vec = dataset_obj if isinstance(dataset_obj, VectorNPZDataset) else None
    model.eval()
    total = torch.zeros((), dtype=torch.float64, device=device)
    n = 0
    met = _Metrics(device)
    for x, y, mask in loader:
        x, y, mask = x.to(device, non_blocking=True), y.to(device, non_blocking=True), mask.to(device, non_blocking=True)
        y_pred = _stack(model(x)[0]) if tta is None else predict_tta(model, x, tta, dataset=vec)
        loss = compute_loss(y_pred, y, mask, use_mask, spec)
        total += loss.double() * x.size(0)
        n += x.size(0)
        met.add(dataset_obj, y, y_pred, mask, use_mask)
        if report is not None:
            report.add(y, y_pred, mask, use_mask)
    return float(total) / max(n, 1), met


def _ema_weights(ema: Optional[WeightEMA]):
    """``ema.swapped()`` for the evaluation passes, or nothing when no EMA is given."""
    if ema is None:
        return contextlib.nullcontext()
    if not isinstance(ema, WeightEMA):
        raise TypeError(f"ema must be a WeightEMA (FusedAdamW.attach_ema) or None, got {type(ema).__name__}")
    return ema.swapped()


@torch.no_grad()
def evaluate(model, loader, device, dataset_obj, use_mask=True, per_channel: bool = False, tta=None, loss: Optional[LossSpec] = None):
    """Reference main.py:150-205.  ``tta``: None, or the ``codes`` of ``predict_tta`` (``"flips"``, ``"d4"``, an iterable): the
    prediction is then the test-time-augmented mean.  ``loss``: the ``LossSpec`` whose value is averaged (None: the reference's).
    A ``VectorNPZDataset`` as ``dataset_obj``: the averaged outputs come back with their channels turned (``predict_tta(dataset=)``),
    the three metrics are pooled over the target channels, and ``per_channel=True`` appends
    ``{"mae": [Cy], "rmse": [Cy], "me": [Cy]}``.  On the averaged weights of ``FusedAdamW.attach_ema()``: call it inside
    ``with ema.swapped():`` (the positional signature is pinned; the two report functions take ``ema=`` themselves)."""
    avg, met = _evaluate(model, loader, device, dataset_obj, use_mask, tta, check_spec(loss))
    return (avg,) + met.result() + ((met.per_channel(),) if per_channel else ())


# ---------------------------------------------------------------------------------------------
# evaluation report (train/get_metrics.py, test.py: the statistics, not the figures)
# ---------------------------------------------------------------------------------------------
_TRANSFORM_IDS = {None: 0, "none": 0, "asinh": 1, "signed_log": 2}


class _ReportBase:
    """What ``EvalReport`` and ``VectorEvalReport`` do alike around their one launch per ``add``.  ``_tables`` holds one tuple per
    ``add`` whose last entry is ``T``."""

    @staticmethod
    def _planes(t: torch.Tensor, what: str) -> torch.Tensor:
        """f32 ``[B,T,C,H,W]`` device tensor whose frames are contiguous planes; anything else is converted / copied once."""
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ops.L.UclstmError(f"EvalReport.add: {what}: a HIP device tensor is required (this package has no CPU path)")
        if t.dim() != 5:
            raise ops.L.UclstmError(f"EvalReport.add: {what}: expected [B,T,C,H,W], got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            t = t.float()
        want, ok = 1, t.stride(0) >= 0 and t.stride(1) >= 0
        for dim in (4, 3, 2):
            ok = ok and (t.size(dim) == 1 or t.stride(dim) == want)
            want *= t.size(dim)
        return t if ok else t.contiguous()

    def _begin(self, device):
        self.device = torch.device(device)
        self._tables = []
        self.last_pointers = None                              # (y_pred, y, mask) addresses handed to the library by the last add()
        self.last_copies = 0                                   # how many of the last add()'s tensors were converted or copied first

    def _inputs(self, y, y_pred, mask, use_mask):
        """``(y_pred, y, mask | None)`` as the kernel reads them; ``last_copies`` counts those that were converted or copied."""
        yp, yt = self._planes(y_pred, "y_pred"), self._planes(y, "y")
        m = self._planes(mask, "mask") if (use_mask and mask is not None) else None
        self.last_copies = int(yp is not y_pred) + int(yt is not y) + int(m is not None and m is not mask)
        return yp, yt, m

    def _rows(self, P, frames) -> int:
        rows = int(ops.L.lib.uclstm_eval_stats_rows(P, frames))
        if rows <= 0:
            raise ops.L.UclstmError(f"{type(self).__name__}.add: bad plane / frame count ({P}, {frames})")
        return rows

    @staticmethod
    def _point(d, yp, yt, m):
        """The pointer and stride fields that ``EvalDesc`` and ``EvalVecDesc`` share."""
        d.y_pred, d.pred_stride_b, d.pred_stride_t = yp.data_ptr(), yp.stride(0), yp.stride(1)
        d.y, d.y_stride_b, d.y_stride_t = yt.data_ptr(), yt.stride(0), yt.stride(1)
        if m is not None:
            d.mask, d.mask_stride_b, d.mask_stride_t = m.data_ptr(), m.stride(0), m.stride(1)

    def _launch(self, entry, name, yp, yt, m):
        """``_describe``, one launch and the bookkeeping of an ``add``: ``T`` is the same in every ``add``."""
        T = yt.shape[1]
        if self._tables and self._tables[0][-1] != T:
            raise ops.L.UclstmError(f"{type(self).__name__}.add: sequences of {T} frames after sequences of {self._tables[0][-1]}")
        d, *written = self._describe(yp, yt, m)
        ops.L.check(entry(d, ops._stream()), name)
        self.last_pointers = (yp.data_ptr(), yt.data_ptr(), None if m is None else m.data_ptr())
        self._tables.append((*written, yt.shape[0], T))

    @staticmethod
    def _read_back(srcs):
        """Every buffer copied to pinned host memory on the current stream, one synchronisation: numpy arrays in the order of ``srcs``."""
        host = [torch.empty(s.shape, dtype=s.dtype, pin_memory=True) for s in srcs]
        for h, s in zip(host, srcs):
            h.copy_(s, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return [h.numpy() for h in host]


class EvalReport(_ReportBase):
    """The statistics of the reference's evaluation scripts, accumulated on the device by ONE kernel per batch
    (``uclstm_eval_stats``): global MAE / RMSE / bias / error std (train/get_metrics.py:188-191), MAE per time step
    (``:281-297``), the three 100-bin histograms (``:317-358``), the ``np.digitize`` count of the target and the balanced
    "up to ``points_per_bin`` random points per target bin" scatter sample (``:210-231``), and the per-frame sums behind
    test.py:333-351.  The defaults are the reference's constants (get_metrics.py:55-59, :317, :354).

    ``add`` launches and returns; ``result`` synchronises once.  ``y_pred`` may be the transposed view the model returns:
    f32 tensors whose ``[C,H,W]`` planes are contiguous are read in place through their batch / time strides (the model's
    output is such a tensor).  Any other input costs one extra pass before the kernel: a tensor of another dtype (a bf16 /
    f16 output) is converted with ``.float()``, one whose planes are not contiguous is copied with ``.contiguous()``;
    ``last_copies`` says how many of the last ``add``'s tensors took that path (0 = everything was read in place).  All sums are f64
    and bitwise reproducible; which pairs the scatter sample keeps is not (the reference's ``np.random.choice`` is unseeded
    too), its per-bin fill counts are exact.
    """

    ROW = 16
    SUMS = ("n", "sum_abs", "sum_sq", "sum")          # the last axis of result()["per_sequence"]

    def __init__(self, dataset_obj, hist_bins=100, hist_range=(-7.5, 7.5), err_range=(-3.0, 3.0), scatter_range=(-8.0, 8.0),
                 scatter_bin_width=0.05, points_per_bin=1000, seed=0, device="cuda"):
        _refuse_vector(dataset_obj, "EvalReport")
        tr = getattr(dataset_obj, "y_transform", None)
        if tr not in _TRANSFORM_IDS:
            raise ValueError(f"EvalReport: unknown y_transform {tr!r}")
        self.transform = _TRANSFORM_IDS[tr]
        self.y_scale = float(getattr(dataset_obj, "y_scale", 1.0))
        self.trans_min, self.trans_max = float(dataset_obj.trans_min), float(dataset_obj.trans_max)
        self.hist_bins = int(hist_bins)
        self.hist_range = (float(hist_range[0]), float(hist_range[1]))
        self.err_range = (float(err_range[0]), float(err_range[1]))
        self.points_per_bin, self.seed = int(points_per_bin), int(seed)
        self.scatter_edges = self.make_scatter_edges(scatter_range, scatter_bin_width)
        if not (1 <= self.hist_bins <= 4096) or not (2 <= len(self.scatter_edges) <= 65536) or self.points_per_bin < 0:
            raise ValueError("EvalReport: hist_bins in [1, 4096], 2..65536 scatter edges and points_per_bin >= 0 are required")
        self._hist = self._dig = self._scatter = None          # device buffers, allocated by the first add()
        self._begin(device)                                    # _tables, per add(): (f64 [rows, ROW] device tensor, B, T)

    @staticmethod
    def make_scatter_edges(scatter_range, width) -> np.ndarray:
        """get_metrics.py:210: ``np.arange(lo, hi + width, width)`` in f64 (321 edges for the defaults)."""
        return np.arange(float(scatter_range[0]), float(scatter_range[1]) + float(width), float(width), dtype=np.float64)

    def _describe(self, yp, yt, m):
        """The descriptor of one launch over validated tensors, and the table it writes (buffers are allocated on first use)."""
        from . import _lib as L
        B, T = yt.shape[:2]
        P = yt.shape[2] * yt.shape[3] * yt.shape[4]
        dev = yt.device
        if self._hist is None:
            nd = len(self.scatter_edges) + 1
            self._hist = torch.zeros((3, self.hist_bins), dtype=torch.int64, device=dev)
            self._dig = torch.zeros(nd, dtype=torch.int64, device=dev)
            self._scatter = torch.zeros((nd, max(self.points_per_bin, 1), 2), dtype=torch.float32, device=dev)
        table = torch.empty((self._rows(P, B * T), self.ROW), dtype=torch.float64, device=dev)
        d = L.EvalDesc()
        self._point(d, yp, yt, m)
        d.B, d.T, d.P = B, T, P
        d.transform, d.y_scale, d.trans_min, d.trans_max = self.transform, self.y_scale, self.trans_min, self.trans_max
        d.table = table.data_ptr()
        d.bins, d.n_edges = self.hist_bins, len(self.scatter_edges)
        (d.hist_lo, d.hist_hi), (d.err_lo, d.err_hi) = self.hist_range, self.err_range
        d.dig_lo, d.dig_w = float(self.scatter_edges[0]), float(self.scatter_edges[1] - self.scatter_edges[0])
        d.hist, d.dig_count = self._hist.data_ptr(), self._dig.data_ptr()
        d.scatter = self._scatter.data_ptr() if self.points_per_bin > 0 else None
        d.seed, d.K = self.seed & 0xFFFFFFFFFFFFFFFF, self.points_per_bin
        return d, table

    @torch.no_grad()
    def add(self, y, y_pred, mask=None, use_mask=False):
        from . import _lib as L
        yp, yt, m = self._inputs(y, y_pred, mask, use_mask)
        if yp.shape != yt.shape or (m is not None and m.shape != yt.shape):
            raise L.UclstmError(f"EvalReport.add: shapes differ: y_pred {tuple(yp.shape)}, y {tuple(yt.shape)}"
                                + ("" if m is None else f", mask {tuple(m.shape)}"))
        self._launch(L.lib.uclstm_eval_stats, "eval_stats", yp, yt, m)

    def result(self) -> dict:
        """One synchronisation: every buffer is copied to pinned host memory on the current stream, then reduced on the host."""
        if not self._tables:
            raise ops.L.UclstmError("EvalReport.result: nothing was added")
        *tables, hist, dig, scatter = self._read_back([t for t, _, _ in self._tables] + [self._hist, self._dig, self._scatter])
        tables = [h.reshape(B, T, -1, self.ROW) for h, (_, B, T) in zip(tables, self._tables)]
        return self.reduce(tables, hist, dig, scatter, hist_range=self.hist_range, err_range=self.err_range,
                           scatter_edges=self.scatter_edges, points_per_bin=self.points_per_bin)

    @staticmethod
    def reduce(tables, hist, dig_count, scatter, *, hist_range, err_range, scatter_edges, points_per_bin) -> dict:
        """Raw tables -> report, on numpy arrays alone.  ``tables``: one f64 ``[B, T, chunks, ROW]`` array per ``add`` (rows as
        ``uclstm_eval_stats`` writes them); ``hist`` ``[3, bins]``, ``dig_count`` ``[n_edges + 1]``, ``scatter``
        ``[n_edges + 1, K, 2]``.  Rows are combined in a fixed order: chunks of a frame, then sequences, then time steps.
        Standard deviations are population ones (``np.std``), from the f64 sums: sqrt(E[x^2] - E[x]^2)."""
        frames = np.concatenate([np.asarray(t, dtype=np.float64).sum(axis=2) for t in tables], axis=0)       # [N, T, ROW] sums
        lo = np.concatenate([np.asarray(t, dtype=np.float64)[..., 8:14:2].min(axis=2) for t in tables], axis=0)
        hi = np.concatenate([np.asarray(t, dtype=np.float64)[..., 9:14:2].max(axis=2) for t in tables], axis=0)
        per_t = frames.sum(axis=0)                                                                           # [T, ROW]
        g = per_t.sum(axis=0)
        n = float(g[0])

        def mean_std(s1, s2):
            if n <= 0:
                return 0.0, 0.0
            mu = s1 / n
            return float(mu), float(math.sqrt(max(s2 / n - mu * mu, 0.0)))

        def ratio(a, b, root=False):
            out = np.divide(a, b, out=np.zeros_like(a), where=b > 0)
            return np.sqrt(out) if root else out

        mean_err, std_err = mean_std(g[3], g[2])
        gt_mean, gt_std = mean_std(g[4], g[5])
        pred_mean, pred_std = mean_std(g[6], g[7])
        mn, mx = lo.min(axis=(0, 1)), hi.max(axis=(0, 1))
        hist = np.asarray(hist).astype(np.int64)
        dig_count = np.asarray(dig_count).astype(np.int64)
        K = int(points_per_bin)
        filled = np.minimum(dig_count, K)
        sc = np.asarray(scatter)
        sel = np.arange(sc.shape[1])[None, :] < filled[:, None] if K > 0 else np.zeros(sc.shape[:2], dtype=bool)
        nt = per_t[:, 0]
        return {
            "n": n,
            "mae": float(g[1] / n) if n > 0 else 0.0,
            "rmse": float(math.sqrt(g[2] / n)) if n > 0 else 0.0,
            "mean_err": mean_err, "std_err": std_err,
            "gt_mean": gt_mean, "gt_std": gt_std, "gt_min": float(mn[0]), "gt_max": float(mx[0]),
            "pred_mean": pred_mean, "pred_std": pred_std, "pred_min": float(mn[1]), "pred_max": float(mx[1]),
            "err_min": float(mn[2]), "err_max": float(mx[2]),
            "per_timestep": {"n": nt.copy(), "mae": ratio(per_t[:, 1], nt), "rmse": ratio(per_t[:, 2], nt, root=True),
                             "mean_err": ratio(per_t[:, 3], nt)},
            "per_sequence": frames[..., :4].copy(),
            "hist_gt": hist[0], "hist_pred": hist[1], "hist_err": hist[2],
            "hist_edges": np.linspace(hist_range[0], hist_range[1], hist.shape[1] + 1),
            "err_edges": np.linspace(err_range[0], err_range[1], hist.shape[1] + 1),
            "scatter_edges": np.asarray(scatter_edges, dtype=np.float64),
            "gt_bin_count": dig_count,
            "scatter_gt": sc[..., 0][sel], "scatter_pred": sc[..., 1][sel],
            "scatter_bin": np.broadcast_to(np.arange(sc.shape[0])[:, None], sc.shape[:2])[sel],
        }


@torch.no_grad()
def evaluate_report(model, loader, device, dataset_obj, use_mask=True, tta=None, loss: Optional[LossSpec] = None, **report_kwargs):
    """``evaluate()``'s loop with an ``EvalReport`` fed from the same ``y_pred``: returns ``(avg_loss, mae, rmse, me, report)``.
    The first four are computed as ``evaluate`` computes them, from the same launches as the report (``report`` is the dict
    of ``EvalReport.result``).  Against a SEPARATE ``evaluate()`` pass they agree as far as ``evaluate`` agrees with itself:
    its loss and metric kernels add block partials with f64 atomics in arrival order, so two passes can differ in the last
    bits (~1e-13 relative); the report's own sums do not have that freedom.  (In deterministic mode, ``ops.deterministic()``, those
    kernels add their block partials in a fixed order and two passes are identical.)  ``tta`` and ``loss``: as in ``evaluate``.
    ``ema=`` (keyword, not passed on to the report): the ``WeightEMA`` of the model's optimiser; the pass then runs inside
    ``ema.swapped()``, on the averaged weights (BatchNorm running statistics as they are), and leaves the weights as they were."""
    averaged = _ema_weights(report_kwargs.pop("ema", None))          # a wrong type is refused here, before anything is built
    _refuse_vector(dataset_obj, "evaluate_report")
    spec = check_spec(loss)
    rep = EvalReport(dataset_obj, device=device, **report_kwargs)
    with averaged:
        avg, met = _evaluate(model, loader, device, dataset_obj, use_mask, tta, spec, rep)
    return (avg,) + met.result() + (rep.result(),)


def _range_per_channel(v, Cy: int, what: str):
    """One ``(lo, hi)`` pair, or one pair per channel -> ``Cy`` pairs of floats."""
    pairs = [v] * Cy if np.ndim(v) == 1 else list(v)
    if len(pairs) != Cy or any(len(p) != 2 for p in pairs):
        raise ValueError(f"VectorEvalReport: {what} must be one (lo, hi) pair or one pair per channel ({Cy})")
    return [(float(lo), float(hi)) for lo, hi in pairs]


class VectorEvalReport(_ReportBase):
    """``EvalReport`` for a ``VectorNPZDataset``: ONE kernel per batch (``uclstm_eval_stats_vec``) gives every target channel the
    statistics of ``EvalReport`` -- channel ``c``'s rows and counts are, bit for bit, those of ``uclstm_eval_stats`` on that channel
    in place -- and, when the dataset has a w- and an h-channel, what a wind model is judged by, which needs both components of
    one pixel: speed error, vector (endpoint) error and direction error.

    Vector quantities are in the IMAGE frame: ``a = s_w * v[w_channel]`` along +column, ``b = s_h * v[h_channel]`` along +row
    (the signs of ``axes``); speed ``sqrt(a^2 + b^2)``, endpoint error ``|p - g|``, direction error the angle from the target to
    the prediction in degrees in (-180, 180], positive from +column towards +row, counted only where both speeds are
    ``>= min_speed``.  Per-pixel values are f32, sums f64 and bitwise reproducible.

    ``hist_range``, ``err_range``, ``scatter_range``: one pair, or one pair per channel (``scatter_bin_width`` is common, and the
    ranges must give the same number of edges).  ``speed_range`` defaults to ``(0, max |hist_range|)`` over the two horizontal
    channels, ``epe_range`` to ``(0, max |err_range|)`` over them.  ``add`` takes what ``EvalReport.add`` takes (the mask is
    ``[B,T,1,H,W]``) and reads it in place under the same conditions; ``result`` synchronises once."""

    ROW, VROW = EvalReport.ROW, 16
    VSUMS = ("n", "sum_abs_ds", "sum_ds_sq", "sum_ds", "sum_speed_gt", "sum_speed_pred", "sum_epe", "sum_epe_sq", "n_dir", "sum_abs_dir",
             "sum_dir", "sum_dir_sq", "max_epe", "max_speed_gt", "max_speed_pred", "reserved")     # the last axis of vector per_sequence

    def __init__(self, dataset_obj, hist_bins=100, hist_range=(-7.5, 7.5), err_range=(-3.0, 3.0), scatter_range=(-8.0, 8.0),
                 scatter_bin_width=0.05, points_per_bin=1000, speed_range=None, epe_range=None, dir_bins=72, min_speed=0.5, seed=0,
                 device="cuda"):
        if not isinstance(dataset_obj, VectorNPZDataset):
            raise TypeError("VectorEvalReport takes a VectorNPZDataset; use EvalReport for a scalar dataset")
        ds = self.ds = dataset_obj
        if ds.y_transform not in _TRANSFORM_IDS:
            raise ValueError(f"VectorEvalReport: unknown y_transform {ds.y_transform!r}")
        Cy = self.Cy = ds.Cy
        self.transform = _TRANSFORM_IDS[ds.y_transform]
        self.hist_bins = int(hist_bins)
        self.hist_range = _range_per_channel(hist_range, Cy, "hist_range")
        self.err_range = _range_per_channel(err_range, Cy, "err_range")
        self.points_per_bin, self.seed = int(points_per_bin), int(seed)
        self.scatter_edges = [EvalReport.make_scatter_edges(r, scatter_bin_width) for r in _range_per_channel(scatter_range, Cy, "scatter_range")]
        n_edges = len(self.scatter_edges[0])
        if any(len(e) != n_edges for e in self.scatter_edges):
            raise ValueError("VectorEvalReport: every channel's scatter_range must give the same number of edges")
        self.pair = (ds.w_channel, ds.h_channel) if ds.w_channel is not None and ds.h_channel is not None else None
        hor = self.pair if self.pair else range(Cy)
        self.speed_range = (0.0, max(abs(v) for c in hor for v in self.hist_range[c])) if speed_range is None else tuple(map(float, speed_range))
        self.epe_range = (0.0, max(abs(v) for c in hor for v in self.err_range[c])) if epe_range is None else tuple(map(float, epe_range))
        self.dir_bins, self.min_speed = int(dir_bins), float(min_speed)
        if not (1 <= self.hist_bins <= 4096) or not (2 <= n_edges <= 65536) or self.points_per_bin < 0:
            raise ValueError("VectorEvalReport: hist_bins in [1, 4096], 2..65536 scatter edges and points_per_bin >= 0 are required")
        if self.speed_range[0] != 0.0 or self.epe_range[0] != 0.0 or not self.speed_range[1] > 0 or not self.epe_range[1] > 0:
            raise ValueError("VectorEvalReport: speed_range and epe_range are (0, hi) with hi > 0")
        if not (1 <= self.dir_bins <= 4096) or not self.min_speed >= 0:
            raise ValueError("VectorEvalReport: dir_bins in [1, 4096] and min_speed >= 0 are required")
        self._hist = self._dig = self._scatter = self._vhist = self._dir = None     # device buffers, allocated by the first add()
        self._begin(device)                                    # _tables, per add(): (table [rows, Cy, ROW], vtable [rows, VROW] | None, B, T)

    def _describe(self, yp, yt, m):
        """The descriptor of one launch over validated tensors, and the tables it writes (buffers are allocated on first use)."""
        from . import _lib as L
        ds, Cy = self.ds, self.Cy
        B, T = yt.shape[:2]
        HW = yt.shape[3] * yt.shape[4]
        dev = yt.device
        nd = len(self.scatter_edges[0]) + 1
        if self._hist is None:
            self._hist = torch.zeros((Cy, 3, self.hist_bins), dtype=torch.int64, device=dev)
            self._dig = torch.zeros((Cy, nd), dtype=torch.int64, device=dev)
            self._scatter = torch.zeros((Cy, nd, max(self.points_per_bin, 1), 2), dtype=torch.float32, device=dev)
            if self.pair:
                self._vhist = torch.zeros((3, self.hist_bins), dtype=torch.int64, device=dev)
                self._dir = torch.zeros(self.dir_bins, dtype=torch.int64, device=dev)
        rows = self._rows(HW, B * T)
        table = torch.empty((rows, Cy, self.ROW), dtype=torch.float64, device=dev)
        vtable = torch.empty((rows, self.VROW), dtype=torch.float64, device=dev) if self.pair else None
        d = L.EvalVecDesc()
        self._point(d, yp, yt, m)
        d.B, d.T, d.Cy, d.transform, d.HW = B, T, Cy, self.transform, HW
        for c, k in enumerate(ds.target_consts()):
            d.consts[c] = k
            (d.hist_lo[c], d.hist_hi[c]), (d.err_lo[c], d.err_hi[c]) = self.hist_range[c], self.err_range[c]
            e = self.scatter_edges[c]
            d.dig_lo[c], d.dig_w[c] = float(e[0]), float(e[1] - e[0])
        d.bins, d.n_edges, d.K, d.dir_bins = self.hist_bins, nd - 1, self.points_per_bin, self.dir_bins
        d.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        d.w_chan, d.h_chan = self.pair if self.pair else (-1, -1)
        d.w_sign, d.h_sign = ((-1 if ds.axes[c][0] == "-" else 1) for c in self.pair) if self.pair else (1, 1)
        d.speed_hi, d.epe_hi, d.min_speed = self.speed_range[1], self.epe_range[1], self.min_speed
        d.table, d.hist, d.dig_count = table.data_ptr(), self._hist.data_ptr(), self._dig.data_ptr()
        d.scatter = self._scatter.data_ptr() if self.points_per_bin > 0 else None
        if self.pair:
            d.vtable, d.vhist, d.dir_hist = vtable.data_ptr(), self._vhist.data_ptr(), self._dir.data_ptr()
        return d, table, vtable

    @torch.no_grad()
    def add(self, y, y_pred, mask=None, use_mask=False):
        from . import _lib as L
        yp, yt, m = self._inputs(y, y_pred, mask, use_mask)
        B, T, _, H, W = yt.shape
        if yp.shape != yt.shape or yt.shape[2] != self.Cy or (m is not None and m.shape != (B, T, 1, H, W)):
            raise L.UclstmError(f"VectorEvalReport.add: y_pred and y must be [B,T,{self.Cy},H,W] and the mask [B,T,1,H,W]: y_pred "
                                f"{tuple(yp.shape)}, y {tuple(yt.shape)}" + ("" if m is None else f", mask {tuple(m.shape)}"))
        self._launch(L.lib.uclstm_eval_stats_vec, "eval_stats_vec", yp, yt, m)

    def result(self) -> dict:
        """One synchronisation: ``{"channels": [EvalReport.reduce of channel c, ...], "vector": reduce_vector(...) | None, "axes"}``."""
        if not self._tables:
            raise ops.L.UclstmError("VectorEvalReport.result: nothing was added")
        n = len(self._tables)
        srcs = [t for t, _, _, _ in self._tables] + [self._hist, self._dig, self._scatter]
        if self.pair:
            srcs += [v for _, v, _, _ in self._tables] + [self._vhist, self._dir]
        host = self._read_back(srcs)
        shapes = [(B, T) for _, _, B, T in self._tables]
        tables = [h.reshape(B, T, -1, self.Cy, self.ROW) for h, (B, T) in zip(host, shapes)]
        hist, dig, scatter = host[n:n + 3]
        channels = [EvalReport.reduce([t[:, :, :, c] for t in tables], hist[c], dig[c], scatter[c], hist_range=self.hist_range[c],
                                      err_range=self.err_range[c], scatter_edges=self.scatter_edges[c], points_per_bin=self.points_per_bin)
                    for c in range(self.Cy)]
        vector = None
        if self.pair:
            vt = [h.reshape(B, T, -1, self.VROW) for h, (B, T) in zip(host[n + 3:], shapes)]
            vector = self.reduce_vector(vt, host[-2], host[-1], speed_range=self.speed_range, epe_range=self.epe_range)
        return {"channels": channels, "vector": vector, "axes": self.ds.axes}

    @staticmethod
    def reduce_vector(vtables, vhist, dir_hist, *, speed_range, epe_range) -> dict:
        """Raw vector tables -> report, on numpy arrays alone.  ``vtables``: one f64 ``[B, T, chunks, VROW]`` array per ``add`` (rows
        as ``uclstm_eval_stats_vec`` writes them); ``vhist`` ``[3, bins]``, ``dir_hist`` ``[dir_bins]``.  Rows are combined as in
        ``EvalReport.reduce``: chunks of a frame, then sequences, then time steps.  ``dir_std`` is the population one."""
        tabs = [np.asarray(t, dtype=np.float64) for t in vtables]
        frames = np.concatenate([np.concatenate([t[..., :12].sum(axis=2), t[..., 12:15].max(axis=2), t[..., 15:].sum(axis=2)], axis=-1)
                                 for t in tabs], axis=0)                                                   # [N, T, VROW]
        per_t = frames[..., :12].sum(axis=0)
        g = per_t.sum(axis=0)
        n, nd = float(g[0]), float(g[8])

        def ratio(a, b):
            return np.divide(a, b, out=np.zeros_like(a), where=b > 0)

        def over(x, m, root=False):
            v = float(x / m) if m > 0 else 0.0
            return math.sqrt(v) if root else v

        mx = frames[..., 12:15].max(axis=(0, 1))
        dir_bias = over(g[10], nd)
        vhist, dir_hist = np.asarray(vhist).astype(np.int64), np.asarray(dir_hist).astype(np.int64)
        return {
            "n": n,
            "speed_mae": over(g[1], n), "speed_rmse": over(g[2], n, root=True), "speed_bias": over(g[3], n),
            "gt_speed_mean": over(g[4], n), "pred_speed_mean": over(g[5], n),
            "epe_mean": over(g[6], n), "epe_rmse": over(g[7], n, root=True), "epe_max": float(mx[0]) if n > 0 else 0.0,
            "n_dir": nd,
            "dir_mae": over(g[9], nd), "dir_bias": dir_bias, "dir_std": math.sqrt(max(over(g[11], nd) - dir_bias * dir_bias, 0.0)),
            "per_timestep": {"n": per_t[:, 0].copy(), "speed_mae": ratio(per_t[:, 1], per_t[:, 0]), "epe_mean": ratio(per_t[:, 6], per_t[:, 0]),
                             "dir_mae": ratio(per_t[:, 9], per_t[:, 8])},
            "per_sequence": frames,
            "hist_speed_gt": vhist[0], "hist_speed_pred": vhist[1], "hist_epe": vhist[2], "hist_dir": dir_hist,
            "speed_edges": np.linspace(speed_range[0], speed_range[1], vhist.shape[1] + 1),
            "epe_edges": np.linspace(epe_range[0], epe_range[1], vhist.shape[1] + 1),
            "dir_edges": np.linspace(-180.0, 180.0, dir_hist.shape[0] + 1),
        }


@torch.no_grad()
def evaluate_vector_report(model, loader, device, dataset_obj, use_mask=True, tta=None, loss: Optional[LossSpec] = None, **report_kwargs):
    """``evaluate()``'s loop for a ``VectorNPZDataset`` with a ``VectorEvalReport`` fed from the same ``y_pred``: returns
    ``(avg_loss, mae, rmse, me, report)``.  The first four are ``evaluate``'s (pooled over the target channels, computed from the same
    launches as the report); ``report`` is the dict of ``VectorEvalReport.result``.  With ``tta`` the averaged outputs come back with
    their channels turned (``predict_tta(dataset=)``).  ``ema=``: as in ``evaluate_report``."""
    averaged = _ema_weights(report_kwargs.pop("ema", None))          # a wrong type is refused here, before anything is built
    rep = VectorEvalReport(dataset_obj, device=device, **report_kwargs)
    with averaged:
        avg, met = _evaluate(model, loader, device, dataset_obj, use_mask, tta, check_spec(loss), rep)
    return (avg,) + met.result() + (rep.result(),)
