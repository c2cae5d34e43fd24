"""Host-side operator layer over the C ABI (include/uclstm.h).

Internal activation format: ``torch.bfloat16`` tensor ``[N, H, W, Cp]`` (NHWC, ``Cp`` = channels
padded to a multiple of 8, padding channels are exactly zero); cell state is ``float32`` in the
same layout.  PyTorch is used here only for device memory, the current HIP stream and autograd
bookkeeping -- every arithmetic kernel is in libuclstm.so.  Nothing in this file runs on CPU
tensors: ``_dev`` raises.
"""
from __future__ import annotations

import ctypes as C
import heapq
import itertools
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib as L

BF16 = torch.bfloat16
F16 = torch.float16
F32 = torch.float32
ACT = (BF16, F16)          # the 16-bit activation / panel dtypes; every operator takes its kernel set from its input's dtype

# Compute dtype of NEW activation tensors at the module boundary (f32 NCHW in -> 16-bit NHWC): bfloat16 by default,
# torch.float16 = the fp16-MFMA twin kernels (BASELINE.json configs[3]).  Downstream operators follow their input's dtype.
_COMPUTE_DTYPE = BF16


def set_compute_dtype(dtype) -> None:
    global _COMPUTE_DTYPE
    if dtype not in ACT:
        raise L.UclstmError(f"compute dtype must be torch.bfloat16 or torch.float16, got {dtype}")
    _COMPUTE_DTYPE = dtype


def get_compute_dtype():
    return _COMPUTE_DTYPE


class compute_dtype:
    """``with ops.compute_dtype(torch.float16): out, _ = model(x)`` -- the forward pass inside runs on the fp16 kernels (the
    backward pass follows the dtype of the saved activations, wherever it runs)."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.prev = _COMPUTE_DTYPE
        set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        set_compute_dtype(self.prev)


# Deterministic mode: every reduction of the training step, the evaluation loop and the optimiser that otherwise ends in float
# atomics (summed in arrival order) takes its ordered form instead -- block partials stored to a scratch buffer, a second launch
# adds them in a fixed order (include/uclstm.h, the *_ordered entry points).  Off by default; UCLSTM_DETERMINISTIC=1 turns it on
# at import.  torch.use_deterministic_algorithms() is NOT consulted: that flag also changes torch.empty and ATen behaviour this
# package does not control, and it does not reach these kernels either way.
_DETERMINISTIC = os.environ.get("UCLSTM_DETERMINISTIC", "0") == "1"


def set_deterministic(on: bool) -> None:
    global _DETERMINISTIC
    _DETERMINISTIC = bool(on)


def is_deterministic() -> bool:
    return _DETERMINISTIC


class deterministic:
    """``with ops.deterministic(): train_step(...)`` -- the work enqueued inside runs on the ordered reductions; the previous
    setting is restored on exit, also when the block raises.  (A captured graph keeps the mode it was captured in.)"""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        self.prev = _DETERMINISTIC
        set_deterministic(self.on)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)


# SyncBatchNorm: with the switch on, every training-mode BatchNorm stage normalises over the batch of ALL ranks of a process group
# (statistics, running statistics and the two mean terms of the backward pass), as the reference does over its one batch -- two
# small f64 all-reduces per stage (uclstm_bn_stats_partial / _from_sums, uclstm_bn_bwd_sums_stage / _finish in include/uclstm.h).
# Every rank must bring the same images per BatchNorm group (DistributedSampler does).  Off by default.
_SYNC_BN = False
_SYNC_BN_GROUP = None              # the process group while the switch is on; None = the default group
_SYNC_BN_CHECKED: set = set()      # (group, n_img, H, W, groups) found equal on every rank


def set_sync_batchnorm(process_group=None) -> None:
    """``True`` -- on, over the default process group; a process group -- on, over that group; ``None`` / ``False`` -- off."""
    global _SYNC_BN, _SYNC_BN_GROUP
    if process_group is None or process_group is False:
        _SYNC_BN, _SYNC_BN_GROUP = False, None
        return
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise L.UclstmError("sync_batchnorm: torch.distributed is not initialised (call init_process_group first)")
    _SYNC_BN, _SYNC_BN_GROUP = True, (None if process_group is True else process_group)


def get_sync_batchnorm():
    """``None`` while the switch is off, otherwise the process group (``True`` stands for the default group)."""
    return None if not _SYNC_BN else (True if _SYNC_BN_GROUP is None else _SYNC_BN_GROUP)


class sync_batchnorm:
    """``with ops.sync_batchnorm(group): train_step(...)`` -- BatchNorm statistics over all ranks of ``group`` (``None``: the
    default group) for the forward passes started inside; the backward pass of such a forward uses the same group wherever it
    runs.  The previous setting is restored on exit, also when the block raises."""

    def __init__(self, process_group=None):
        self.group = True if process_group is None else process_group

    def __enter__(self):
        self.prev = get_sync_batchnorm()
        set_sync_batchnorm(self.group)
        return self

    def __exit__(self, *exc):
        global _SYNC_BN, _SYNC_BN_GROUP
        _SYNC_BN, _SYNC_BN_GROUP = self.prev is not None, (None if self.prev in (None, True) else self.prev)


def _sync_bn_check_equal(group, n_img: int, H: int, W: int, groups: int) -> int:
    """World size of ``group``, after making sure ONCE per shape that every rank brings the same images and plane size per
    BatchNorm group (one small host-side collective; afterwards nothing here touches the host).  A shape seen for the first
    time must be new on every rank at the same step, or the ranks disagree about who takes part in the collective -- equal work
    per rank, which the scheme needs anyway, guarantees it."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    key = (group, n_img, H, W, groups)
    if key not in _SYNC_BN_CHECKED:
        mine = (int(n_img), int(H), int(W), int(groups))
        seen = [None] * world
        dist.all_gather_object(seen, mine, group=group)
        if any(tuple(s) != mine for s in seen):
            raise L.UclstmError("sync_batchnorm: every rank must bring the same (images, H, W, BatchNorm groups) per stage, got "
                                + ", ".join(f"rank {r}: {tuple(s)}" for r, s in enumerate(seen)))
        _SYNC_BN_CHECKED.add(key)
    return world


def _sync_bn_all_reduce(t: torch.Tensor, group, what: str) -> None:
    """Sum of ``t`` (f64) over the ranks, ordered into the current stream: RCCL's stream waits for the current stream and the
    current stream for the collective (no host block); gloo copies through the host and blocks it (tests)."""
    import torch.distributed as dist
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append(("collective", what, t.numel() * t.element_size()))
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def _bn_bwd_sums_over_ranks(sums: torch.Tensor, sync, variant: str) -> torch.Tensor:
    """The backward sums of all ranks in the form the apply kernels take (``sums`` itself stays local for the parameter
    gradients).  ``sync`` = (group, world) of the forward pass; ``variant`` ("plain" / "pool" / "head") goes to LAUNCH_LOG."""
    group, world = sync
    sums64 = torch.empty(sums.shape, dtype=torch.float64, device=sums.device)
    sums_dz = torch.empty_like(sums)
    n = sums.numel()
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append(("syncbn", "bn_bwd_sums_stage", variant))
    L.check(L.lib.uclstm_bn_bwd_sums_stage(_p(sums), _p(sums64), n, _stream()), "bn_bwd_sums_stage")
    _sync_bn_all_reduce(sums64, group, "bn_bwd_sums")
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append(("syncbn", "bn_bwd_sums_finish", variant))
    L.check(L.lib.uclstm_bn_bwd_sums_finish(_p(sums64), 1.0 / world, _p(sums_dz), n, _stream()), "bn_bwd_sums_finish")
    return sums_dz


def _k(t: torch.Tensor):
    """Kernel set (bf16 / fp16 twins) for a 16-bit activation tensor."""
    return L.kernels(t.dtype)


def cpad(c: int) -> int:
    return (c + 7) // 8 * 8


def kseg(c: int) -> int:
    return (c + 63) // 64 * 64


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t: torch.Tensor, dtype=None, what: str = "tensor") -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.UclstmError(f"{what}: a HIP device tensor is required (this package has no CPU path)")
    if dtype is not None and (t.dtype not in dtype if isinstance(dtype, tuple) else t.dtype != dtype):
        raise L.UclstmError(f"{what}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.UclstmError(f"{what}: must be contiguous")
    return t


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


# Optional per-launch timing of the MFMA kernels (bench.py's roofline leg): when PROFILE is a list every GEMM launch
# is bracketed by HIP events on the launch stream and (kernel, algorithmic flops, start, stop) is appended.
PROFILE: Optional[list] = None


# Optional record of which forward-family kernel each launch takes (uclstm_igemm_fwd_shape: 0 / 1 per-tap shapes, 2 patch loop,
# 3 ring kernel, 4 flat kernel): tests set it to a list to assert that a parity case exercised the kernel it is meant for.
SHAPE_LOG: Optional[list] = None
# Same, as (epilogue, shape) pairs -- epilogue 0 store, 1 fused ConvLSTM cell, 2 split-K partial tiles: the BASELINE-shape
# parity tests assert that the fused-cell, split-K and patch kernels the benchmark runs were the ones compared.
KERNEL_LOG: Optional[list] = None


# Same again with the geometry, for the full-size property tests: ("fwd", epilogue, shape, image width, N), ("wgrad", shape,
# N, Ktot, pixel-range slabs) and ("split", what, image ranges) for a launch cut at the 2-GiB descriptor range.
LAUNCH_LOG: Optional[list] = None


# Optional record of what the ConvLSTM recurrence stored per step: when it is a list, ConvLSTMSeq.forward and
# convlstm_group_forward (once per member) append ("fwd", h_hist, c_hist, gates) and ConvLSTMSeq.backward appends
# ("bwd", dgates) after its loop -- the tensors themselves, not copies.  tests/test_gpu_recurrence.py checks every step of a
# sequence against an f64 cell on these stored inputs.  None (the default): nothing is recorded and no launch changes.
RECURRENCE_TRACE: Optional[list] = None


def _log_shape(d) -> None:
    if SHAPE_LOG is not None or KERNEL_LOG is not None or LAUNCH_LOG is not None:
        shp = int(L.lib.uclstm_igemm_fwd_shape(C.byref(d)))
        if SHAPE_LOG is not None:
            SHAPE_LOG.append(shp)
        if KERNEL_LOG is not None:
            KERNEL_LOG.append((int(d.epi), shp))
        if LAUNCH_LOG is not None:
            LAUNCH_LOG.append(("fwd", int(d.epi), shp, int(d.W), int(d.N)))


# The reductions that end in float atomics by default and in an ordered second launch in deterministic mode are recorded in
# LAUNCH_LOG as ("reduce", kind), so that a test can assert which path a step took.  The weight-gradient unpack is recorded only
# where its slabs are spread over several slab groups (the only place it is atomic); every other unpack is ordered in both modes.
ATOMIC_KINDS = ("colsum", "outconv_bwd", "bn_head_bwd_reduce", "unpack_atomic", "loss_fwd", "sumsq", "metric_sums")
ORDERED_KINDS = tuple((k if k != "unpack_atomic" else "unpack") + "_ordered" for k in ATOMIC_KINDS)


def _log_reduce(kind: str) -> None:
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append(("reduce", kind))


# Same for the HBM-bound kernels (BatchNorm passes, pooling, LSTM point-wise): (kernel, algorithmic BYTES, start, stop, note).
PROFILE_HBM: Optional[list] = None


def _timed_hbm(kind: str, nbytes: float, launch) -> None:
    if PROFILE_HBM is None:
        launch()
        return
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    PROFILE_HBM.append((kind, nbytes, e0, e1, ""))


_SHAPE_NAMES = {0: "pertap128x128", 1: "pertap64x256", 2: "patch128x256", 3: "ring64", 4: "flat128x256"}


def _kernel_kind(kind: str, d) -> str:
    """Profile key of a forward-family launch: epilogue family + the kernel the library picks for this descriptor (the
    rocprofv3 name is igemm_fwd_kernel<epilogue, shape, sources> / igemm_fwd_c64_kernel), so that bench.py's roofline leg
    prices each KERNEL, not a mix of MFMA-bound 3x3 launches and HBM-bound 1x1 / 2x2 ones."""
    if PROFILE is None:
        return kind
    return f"{kind}[{_SHAPE_NAMES.get(int(L.lib.uclstm_igemm_fwd_shape(C.byref(d))), '?')}]"


def _timed(kind: str, flops: float, launch, note: str = "", nbytes: float = 0.0) -> None:
    """``nbytes``: ALGORITHMIC HBM bytes of the launch -- every operand read once, the result written once (split-K /
    pixel-range slabs counted as ONE result) -- the partner of the PMC traffic figure in bench.py's roofline leg."""
    if PROFILE is None:
        launch()
        return
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    PROFILE.append((kind, flops, e0, e1, note, float(nbytes)))


def _nb(*tensors) -> int:
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


# ---------------------------------------------------------------------------------------------
# descriptors
# ---------------------------------------------------------------------------------------------
class SrcView:
    """One input of a convolution: NHWC bf16 tensor placed at (offY, offX) in the output frame."""

    def __init__(self, t: torch.Tensor, offY: int = 0, offX: int = 0):
        _dev(t, ACT, "conv source")
        assert t.dim() == 4 and t.shape[3] % 8 == 0
        if offY < 0 or offX < 0:
            # measured: a source that overhangs the output frame reads out of range in the input-gradient / weight-gradient
            # kernels (garbage, not zeros).  modules.Up crops such a source before it gets here.
            raise L.UclstmError("conv source offsets must be >= 0 (a source is placed INSIDE the output frame)")
        self.t, self.offY, self.offX = t, offY, offX

    def fill(self, s: L.Src):
        s.ptr = self.t.data_ptr()
        s.C = self.t.shape[3]
        s.Hs, s.Ws = self.t.shape[1], self.t.shape[2]
        s.offY, s.offX = self.offY, self.offX


def _fill_seg(sg: L.Seg, t: torch.Tensor, n_begin: int, n_end: int, c_off: int = 0, scale: int = 1, oy: int = 0, ox: int = 0):
    sg.ptr = t.data_ptr()
    sg.n_begin, sg.n_end = n_begin, n_end
    sg.C, sg.c_off = t.shape[3], c_off
    sg.Hd, sg.Wd = t.shape[1], t.shape[2]
    sg.scale, sg.oy, sg.ox = scale, oy, ox


def conv_pack_desc(Co: int, Ci_total: int, c_valid: Sequence[int], c_pad: Sequence[int], k: int = 3) -> L.PackDesc:
    """Forward panel of a k x k conv whose input is the channel concat of the sources (train/unet.py:70,:98).  THE builder of both
    models' convolutions: ``bytes(desc)`` is the key of the panel cache and of the look-ahead plan (pack_weights).  One source:
    ``choff[1]`` is 0 as in every other one-source descriptor here (csrc/pack.hip reads it only for columns of source 1, and with
    ``kseg[1] == 0`` there are none)."""
    d = L.PackDesc()
    taps, two = k * k, len(c_valid) > 1
    d.N, d.taps, d.nsrc = cpad(Co), taps, len(c_valid)
    d.kseg[0], d.kseg[1] = kseg(c_pad[0]), (kseg(c_pad[1]) if two else 0)
    d.cvalid[0], d.cvalid[1] = c_valid[0], (c_valid[1] if two else 0)
    d.choff[0], d.choff[1] = 0, (c_valid[0] if two else 0)
    d.Ktot = taps * (d.kseg[0] + d.kseg[1])
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, Co, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = Ci_total * taps, taps, 1, 0
    return d


def conv_dgrad_pack_desc(Co: int, Ci_total: int, c_valid_s: int) -> L.PackDesc:
    """Input-gradient panel for ONE source: rows = its input channels, K = (flipped tap, out channel)."""
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = cpad(c_valid_s), 9, 1
    d.kseg[0], d.kseg[1] = kseg(cpad(Co)), 0
    d.cvalid[0], d.cvalid[1] = Co, 0
    d.choff[0], d.choff[1] = 0, 0
    d.Ktot = 9 * d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, c_valid_s, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 1
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = 9, Ci_total * 9, 1, 0
    return d


def im2col_pack_desc(Co: int, Ci: int, Kp: int) -> L.PackDesc:
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = cpad(Co), 1, 1
    d.kseg[0], d.kseg[1] = kseg(Kp), 0
    d.cvalid[0], d.cvalid[1] = 9 * Ci, 0
    d.choff[0] = d.choff[1] = 0
    d.Ktot = d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, Co, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IM2COL, 9, Ci, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = Ci * 9, 9, 1, 0
    return d


def lstm_pack_desc(Hd: int, Cx: int, ksize: int = 3) -> L.PackDesc:
    """Gate-interleaved forward panel of the ConvLSTM gate conv [4Hd, Cx+Hd, k, k] (train/unet.py:19)."""
    taps = ksize * ksize
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = 64 * ((Hd + 15) // 16), taps, 2
    d.kseg[0], d.kseg[1] = kseg(cpad(Cx)), kseg(cpad(Hd))
    d.cvalid[0], d.cvalid[1] = Cx, Hd
    d.choff[0], d.choff[1] = 0, Cx
    d.Ktot = taps * (d.kseg[0] + d.kseg[1])
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_LSTM, Hd, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = (Cx + Hd) * taps, taps, 1, 0
    return d


def lstm_half_pack_desc(Hd: int, Cx: int, half: str, ksize: int = 3) -> L.PackDesc:
    """One half of the gate convolution as its own gate-interleaved panel: ``half='x'`` = W_x (input channels [0, Cx) of
    train/unet.py:19's conv, applied to x_t), ``'h'`` = W_h (channels [Cx, Cx+Hd), applied to h_{t-1}).  W_x * x_t does not
    depend on the recurrence, so it is hoisted out of the time loop of train/unet.py:55-57 and computed for all timesteps
    by one GEMM; the serial step then carries only W_h * h_{t-1} (half the K, half the weight traffic per step)."""
    taps = ksize * ksize
    cs = Cx if half == "x" else Hd
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = 64 * ((Hd + 15) // 16), taps, 1
    d.kseg[0], d.kseg[1] = kseg(cpad(cs)), 0
    d.cvalid[0], d.cvalid[1] = cs, 0
    d.choff[0], d.choff[1] = (0 if half == "x" else Cx), 0
    d.Ktot = taps * d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_LSTM, Hd, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = (Cx + Hd) * taps, taps, 1, 0
    return d


def lstm_dgrad_pack_desc(Hd: int, Cx: int, c_valid_s: int, ksize: int = 3) -> L.PackDesc:
    """Input-gradient panel of the gate conv for one source (x or h); K = (flipped tap, gate*Hd_p + hc)."""
    taps = ksize * ksize
    Hdp = cpad(Hd)
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = cpad(c_valid_s), taps, 1
    d.kseg[0], d.kseg[1] = kseg(4 * Hdp), 0
    d.cvalid[0], d.cvalid[1] = 4 * Hd, 0
    d.choff[0] = d.choff[1] = 0
    d.Ktot = taps * d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, c_valid_s, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_GATES, Hdp, Hd, 1
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = taps, (Cx + Hd) * taps, 1, 0
    return d


def lstm_wgrad_unpack_desc(Hd: int, Cx: int, ksize: int = 3) -> L.PackDesc:
    """Panel-gradient layout of the gate conv: rows = gate*Hd_p + hc (the dgates channel order)."""
    taps = ksize * ksize
    Hdp = cpad(Hd)
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = 4 * Hdp, taps, 2
    d.kseg[0], d.kseg[1] = kseg(cpad(Cx)), kseg(Hdp)
    d.cvalid[0], d.cvalid[1] = Cx, Hd
    d.choff[0], d.choff[1] = 0, Cx
    d.Ktot = taps * (d.kseg[0] + d.kseg[1])
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_TAPMAJOR, Hd, Hdp
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap = (Cx + Hd) * taps, taps, 1
    d.stride_ntap = Hd * (Cx + Hd) * taps
    return d


def convt_pack_desc(Ci: int, Co: int) -> L.PackDesc:
    """Forward panel of ConvTranspose2d(Ci, Co, 2, stride 2): rows (tap, co), K = ci (weight [Ci,Co,2,2], train/unet.py:90)."""
    Cop = cpad(Co)
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = 4 * Cop, 1, 1
    d.kseg[0], d.kseg[1] = kseg(cpad(Ci)), 0
    d.cvalid[0], d.cvalid[1] = Ci, 0
    d.choff[0] = d.choff[1] = 0
    d.Ktot = d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_TAPMAJOR, Co, Cop
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = 4, Co * 4, 0, 1
    return d


def convt_dgrad_pack_desc(Ci: int, Co: int) -> L.PackDesc:
    d = L.PackDesc()
    d.N, d.taps, d.nsrc = cpad(Ci), 4, 1
    d.kseg[0], d.kseg[1] = kseg(cpad(Co)), 0
    d.cvalid[0], d.cvalid[1] = Co, 0
    d.choff[0] = d.choff[1] = 0
    d.Ktot = 4 * d.kseg[0]
    d.n_mode, d.n_valid, d.n_cp = L.NMODE_IDENTITY, Ci, 0
    d.k_mode, d.k_hdp, d.k_hd, d.tap_flip = L.KMODE_IDENTITY, 0, 0, 0
    d.stride_n, d.stride_k, d.stride_tap, d.stride_ntap = Co * 4, 4, 1, 0
    return d


# Inference-time panel cache.  There is no module-global cache: a caller that owns frozen weights (streaming.
# StreamingPredictor) creates a ``PanelCache`` and makes it current around its forward calls; the panels live exactly as long
# as that object (a captured HIP graph has their addresses baked in, so they must not be freed under it).  Entries are
# validated by the weight tensor's version AND by ``WEIGHTS_EPOCH``, which the fused optimiser bumps on every step: it updates
# parameters through raw pointers, which does not change tensor versions.
WEIGHTS_EPOCH = 0


def weights_changed() -> None:
    """Called by code that rewrites parameter storage behind autograd's back (optim.FusedAdamW.step)."""
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1


class PanelCache:
    """Packed panels of frozen weights, keyed by (storage address, element offset, pack descriptor)."""

    def __init__(self):
        self.entries: dict = {}
        self.epoch = WEIGHTS_EPOCH

    def stale(self) -> bool:
        return self.epoch != WEIGHTS_EPOCH

    def clear(self) -> None:
        self.entries.clear()
        self.epoch = WEIGHTS_EPOCH

    def __enter__(self):
        global _ACTIVE_CACHE
        self._prev = _ACTIVE_CACHE
        _ACTIVE_CACHE = self
        return self

    def __exit__(self, *exc):
        global _ACTIVE_CACHE
        _ACTIVE_CACHE = self._prev


_ACTIVE_CACHE: Optional[PanelCache] = None


# Look-ahead packing for training steps (engine.train_step): the weights only change in the optimiser step, so every panel of
# a step -- the forward panels and, 15 ms later, the input-gradient panels -- can be packed at the START of the step.  The
# list of pack calls of one step is remembered; at the start of the next step all of them are replayed on the side stream
# (HBM-bound 10-80 us kernels, ~1.5 ms per step in a row on the main stream before), each followed by an event, and
# pack_weights() on the main stream turns into a wait for that event.  A call that the plan does not know packs in line.
PREPACK = os.environ.get("UCLSTM_PREPACK", "1") != "0"
_PACK_PLAN: list = []          # [(key, desc copy, weight, elem_offset)] in call order, recorded during the previous step
_PACK_READY: dict = {}         # key -> (panel, event) produced by prepack_begin() for the current step
_PACK_RECORDING = False


PACK_BATCHED = os.environ.get("UCLSTM_PACK_BATCHED", "1") != "0"


PACK_SEGMENTS = tuple(float(x) for x in os.environ.get("UCLSTM_PACK_SEGMENTS", "0.02,0.08,0.2,0.35,0.5,0.65,0.8").split(",") if x)


def pack_segments(sizes: Sequence[int], fractions: Sequence[float]) -> List[int]:
    """Segment index of every panel (in order of first use): panel i belongs to segment s when the bytes BEFORE it have
    reached ``fractions[s - 1]`` of the total (and not yet ``fractions[s]``); non-decreasing, segment 0 is never empty."""
    total, run, seg_of = float(sum(sizes)), 0, []
    for sz in sizes:
        seg_of.append(sum(1 for f in fractions if run >= f * total))
        run += sz
    return seg_of


class _PackBatch:
    """All look-ahead panels of a step as a few launches per kernel family (uclstm_pack_weights_batched).

    The job table (descriptors, weight and panel pointers, block ranges) is built once and lives on the device; the panels
    are persistent, which is safe inside train_step: the step's packing waits for everything the main stream has been
    given (side.wait_stream(main) in prepack_begin), i.e. for the last reader of the previous step.

    The panels are cut, in order of first use, into segments at the cumulative byte fractions PACK_SEGMENTS; a segment is one
    launch per family followed by an event, so the step's first convolutions wait for the first few per cent of the bytes
    only.  (Holding the later segments back until the main stream reaches the MFMA-bound layers was tried and measured no
    different: packing is ~0.55 ms of HBM traffic per step and costs about that wherever it runs, profiles/round2_notes.md.)
    """

    def __init__(self, items):
        self.sig = tuple(key for key, _, _, _ in items)
        self.panels, self.keep, self.segments = {}, [], []            # segments: [[(dtype, fam, byte offset, njobs, blocks)]]
        dev = items[0][2].device
        seg_of = pack_segments([desc.N * desc.Ktot for _, desc, _, _ in items], PACK_SEGMENTS)
        jobs_all = []
        for n, seg in enumerate(sorted(set(seg_of))):
            groups: dict = {}
            for (key, desc, w, off), sg in zip(items, seg_of):
                if sg != seg:
                    continue
                wp = torch.empty((desc.N, desc.Ktot), dtype=key[3], device=dev)
                job = L.PackJob()
                fam = L.lib.uclstm_pack_job_init(C.byref(job), C.byref(desc), C.c_void_p(w.data_ptr() + 4 * off), _p(wp), 0)
                L.check(min(fam, 0), "pack_job_init")
                groups.setdefault((key[3], fam), []).append(job)
                self.panels[key] = (wp, n)
                self.keep.append(w)
            launches = []
            for (dtype, fam), jobs in groups.items():
                b0, first = 0, len(jobs_all)
                for j in jobs:
                    j.block0 = b0
                    b0 += j.nblocks
                    jobs_all.append(j)
                launches.append((dtype, fam, first * C.sizeof(L.PackJob), len(jobs), b0))
            self.segments.append(launches)
        arr = (L.PackJob * len(jobs_all))(*jobs_all)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.events: list = [None] * len(self.segments)

    def launch(self, side) -> None:
        """Launch every segment on ``side``; events[s] is recorded behind segment s."""
        base, st = self.table.data_ptr(), C.c_void_p(side.cuda_stream)
        for sg, launches in enumerate(self.segments):
            for dtype, fam, byte_off, n, blocks in launches:
                L.check(L.kernels(dtype).uclstm_pack_weights_batched(C.c_void_p(base + byte_off), n, fam, blocks, st), "pack_weights_batched")
            self.events[sg] = torch.cuda.Event()
            self.events[sg].record(side)

    def panel(self, key, main) -> torch.Tensor:
        wp, sg = self.panels[key]
        main.wait_event(self.events[sg])
        return wp


_PACK_BATCH: Optional[_PackBatch] = None


def prepack_begin() -> None:
    """Start of a training step whose parameters will not change before its backward pass has run."""
    global _PACK_RECORDING, _PACK_PLAN, _PACK_BATCH
    _PACK_READY.clear()
    _PACK_RECORDING = False
    if not PREPACK:
        return
    plan, _PACK_PLAN = _PACK_PLAN, []
    _PACK_RECORDING = True
    if not plan:
        return
    dev = plan[0][2].device
    main, side = torch.cuda.current_stream(dev), side_stream(dev)
    if PACK_BATCHED:
        items, seen = [], set()
        for it in plan:
            if it[0] not in seen and it[2].data_ptr() == it[0][0]:
                seen.add(it[0])
                items.append(it)
        if not items:
            return
        if _PACK_BATCH is None or _PACK_BATCH.sig != tuple(it[0] for it in items):
            _PACK_BATCH = _PackBatch(items)          # panels allocated on the main stream: their later reuse is ordered there
        side.wait_stream(main)                       # the optimiser step that produced these weights + the panels' last readers
        _PACK_BATCH.launch(side)
        for key in _PACK_BATCH.panels:
            _PACK_READY[key] = _PACK_BATCH
        return

    def pack_all():
        for key, desc, w, off in plan:
            if key in _PACK_READY or w.data_ptr() != key[0]:
                continue
            wp = torch.empty((desc.N, desc.Ktot), dtype=key[3], device=w.device)
            L.check(L.kernels(key[3]).uclstm_pack_weights(C.byref(desc), C.c_void_p(w.data_ptr() + 4 * off), _p(wp), _stream()), "pack_weights")
            wp.record_stream(main)
            ev = torch.cuda.Event()
            ev.record(side)
            _PACK_READY[key] = (wp, ev)

    _on_side(dev, pack_all)                      # after the optimiser step that produced these weights


def prepack_end() -> None:
    """End of the step (before the optimiser changes the weights): panels packed ahead are no longer valid."""
    global _PACK_RECORDING
    _PACK_READY.clear()
    _PACK_RECORDING = False


def pack_weights(desc: L.PackDesc, w: torch.Tensor, elem_offset: int = 0, dtype=BF16, lookahead: bool = True) -> torch.Tensor:
    """f32 reference-layout weight -> 16-bit panel of ``dtype`` (the dtype of the activations it will multiply).
    ``lookahead=False``: ``w`` is a temporary derived from a parameter inside the step (resnet.s2_dgrad_weight), not a parameter: the
    look-ahead plan, which replays from the tensors it recorded at the start of the NEXT step, must not know it."""
    _dev(w, F32, "weight")
    key = None
    if _PACK_RECORDING and lookahead:
        key = (w.data_ptr(), elem_offset, bytes(desc), dtype)
        d2 = L.PackDesc()
        C.memmove(C.byref(d2), C.byref(desc), C.sizeof(L.PackDesc))
        _PACK_PLAN.append((key, d2, w, elem_offset))
        hit = _PACK_READY.get(key)
        if hit is not None:
            main = torch.cuda.current_stream(w.device)
            if hit is _PACK_BATCH:
                return hit.panel(key, main)
            main.wait_event(hit[1])
            return hit[0]
        key = None
    cache = _ACTIVE_CACHE
    if cache is not None:
        if cache.stale():
            raise L.UclstmError("PanelCache: the weights changed (optimiser step) while a panel cache was current; its owner "
                                "must drop it first (StreamingPredictor does so in step())")
        key = (w.data_ptr(), elem_offset, bytes(desc), dtype)
        hit = cache.entries.get(key)
        if hit is not None and hit[0] == w._version:
            return hit[1]
    wp = torch.empty((desc.N, desc.Ktot), dtype=dtype, device=w.device)
    L.check(L.kernels(dtype).uclstm_pack_weights(C.byref(desc), C.c_void_p(w.data_ptr() + 4 * elem_offset), _p(wp), _stream()), "pack_weights")
    if key is not None:
        cache.entries[key] = (w._version, wp)
    return wp


def pack_bias(desc: L.PackDesc, b: torch.Tensor) -> torch.Tensor:
    _dev(b, F32, "bias")
    if desc.n_mode == L.NMODE_IDENTITY and desc.N == desc.n_valid == b.numel() and b.is_contiguous() and b.data_ptr() % 16 == 0:
        return b.detach()          # panel-row order == channel order and no padding rows: the bias IS its panel (no kernel)
    cache, key = _ACTIVE_CACHE, None
    if cache is not None and not cache.stale():              # frozen weights (StreamingPredictor): once, like the weight panels
        key = ("bias", b.data_ptr(), bytes(desc))
        hit = cache.entries.get(key)
        if hit is not None and hit[0] == b._version:
            return hit[1]
    bp = torch.empty((desc.N,), dtype=F32, device=b.device)
    L.check(L.lib.uclstm_pack_bias(C.byref(desc), _p(b), _p(bp), _stream()), "pack_bias")
    if key is not None:
        cache.entries[key] = (b._version, bp)
    return bp


def unpack_wgrad(desc: L.PackDesc, dwp: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """dwp: f32 panel gradient [N, Ktot] or its per-pixel-range slabs [splits, N, Ktot] (added up here)."""
    grad = torch.empty_like(like, dtype=F32, memory_format=torch.contiguous_format)
    _unpack_wgrad_launch(desc, dwp, grad, 0)
    return grad


def _unpack_wgrad_launch(desc: L.PackDesc, dwp: torch.Tensor, grad: torch.Tensor, accumulate: int) -> None:
    """grad = (accumulate ? grad : 0) + sum of the slabs of dwp, on the current stream.  Deterministic mode: the ordered form,
    with a scratch row per slab group where the library splits the slabs (allocated on the current stream, freed to it)."""
    ns, st = _slabs_of(dwp)
    if _DETERMINISTIC:
        groups = int(L.lib.uclstm_unpack_wgrad_ordered_groups(C.byref(desc), ns))
        if groups < 1:
            raise L.UclstmError(f"unpack_wgrad_ordered_groups: code {groups}")
        scratch = torch.empty((groups, desc.N * desc.Ktot), dtype=F32, device=grad.device) if groups > 1 else None
        if groups > 1:
            _log_reduce("unpack_ordered")
        L.check(L.lib.uclstm_unpack_wgrad_ordered(C.byref(desc), _p(dwp), ns, st, _p(scratch), _p(grad), accumulate, _stream()),
                "unpack_wgrad_ordered")
        return
    if LAUNCH_LOG is not None and accumulate and int(L.lib.uclstm_unpack_wgrad_ordered_groups(C.byref(desc), ns)) > 1:
        _log_reduce("unpack_atomic")
    L.check(L.lib.uclstm_unpack_wgrad(C.byref(desc), _p(dwp), ns, st, _p(grad), accumulate, _stream()), "unpack_wgrad")


def _slabs_of(dwp: torch.Tensor) -> Tuple[int, int]:
    return (dwp.shape[0], dwp.stride(0)) if dwp.dim() == 3 else (1, 0)


# ---------------------------------------------------------------------------------------------
# weight gradients on a side stream
# ---------------------------------------------------------------------------------------------
# The weight-gradient GEMM of a layer is not on the critical path of backward (only the optimiser needs it), while the
# HBM-bound kernels between the input-gradient GEMMs (BatchNorm backward, pool, point-wise LSTM, packing) leave the MFMA
# pipes idle.  When the parameter already owns a gradient buffer (``optim.FlatParams`` / ``zero_grad(set_to_none=False)``),
# the weight-gradient GEMM + its unpack-ACCUMULATE into ``weight.grad`` are enqueued on a second HIP stream and the
# autograd function returns ``None`` for that parameter; the main stream re-joins at the end of the backward pass
# (autograd engine callback), before anything can read the gradients.  ``GRAD_SIDE_HOOKS`` lets data-parallel code learn
# that a parameter's gradient has been enqueued (the hook runs with the side stream current).
ASYNC_WGRAD = os.environ.get("UCLSTM_ASYNC_WGRAD", "1") != "0"
BN_RUNNING_ON_SIDE = os.environ.get("UCLSTM_BN_RUNNING_ON_SIDE", "1") != "0"     # running-statistics recursion on the second stream
_FWD_SIDE_PENDING: set = set()


def join_forward_side(device) -> None:
    """Make the current stream wait for forward-pass work that was put on the second stream (BatchNorm running statistics).
    Called where such results become observable: at the end of a module's public forward, before evaluation-mode
    BatchNorm reads the running statistics; the backward pass joins the second stream anyway."""
    key = str(device)
    if key in _FWD_SIDE_PENDING:
        _FWD_SIDE_PENDING.discard(key)
        torch.cuda.current_stream(device).wait_stream(side_stream(device))


PARAM_GRADS_ON_SIDE = os.environ.get("UCLSTM_PARAM_GRADS_ON_SIDE", "1") != "0"   # BatchNorm parameter gradients on the weight-gradient stream
HOIST_X = os.environ.get("UCLSTM_HOIST_X", "0") == "1"               # x half of the ConvLSTM gate conv as one GEMM over all T (off: measured slower)
POOL_SKIP = os.environ.get("UCLSTM_POOL_SKIP", "1") != "0"            # skip-connection gradient added inside max-pool backward
DIRECT_GRADS = os.environ.get("UCLSTM_DIRECT_GRADS", "1") != "0"     # small parameter gradients written by the backward kernels
GRAD_SIDE_HOOKS: list = []
_WGRAD_OVERLAPPED = False      # True while a weight-gradient GEMM is being enqueued on the side stream
_SIDE_STREAMS = {}
_LAUNCH_STREAMS = {}
_SIDE_STREAM_PROBES = {}       # device -> number of candidate streams tried (diagnostics)
_JOIN_PENDING = set()


def _streams_overlap(main: "torch.cuda.Stream", cand: "torch.cuda.Stream", spin_us: int = 300) -> bool:
    """True when a kernel on ``cand`` executes while one on ``main`` is still running.  The HIP runtime multiplexes
    streams onto a few hardware queues; two streams that share one are serialised, and which ones collide depends on
    every stream created before (an RCCL communicator shifts the assignment: measured 37.7 -> 42.0 ms per step with
    the weight gradients silently serialised behind the main stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    main.synchronize()
    cand.synchronize()
    e0.record(main)
    L.check(L.lib.uclstm_stream_spin(spin_us, C.c_void_p(main.cuda_stream)), "stream_spin")
    L.check(L.lib.uclstm_stream_spin(spin_us, C.c_void_p(cand.cuda_stream)), "stream_spin")
    e1.record(cand)
    cand.synchronize()
    main.synchronize()
    return e0.elapsed_time(e1) < 1.5e-3 * spin_us


def _pick_stream(device, others) -> tuple:
    """(stream, tried): the first of up to eight fresh streams that demonstrably runs concurrently with every stream in
    ``others``; the first candidate (and a warning) when none does."""
    cands = []
    if os.environ.get("UCLSTM_SIDE_STREAM_PROBE", "1") != "0" and not torch.cuda.is_current_stream_capturing():
        # first launch of the spin kernel outside the timed comparison (code-object load)
        L.check(L.lib.uclstm_stream_spin(1, C.c_void_p(others[0].cuda_stream)), "stream_spin")
        for _ in range(8):
            cands.append(torch.cuda.Stream(device=device))
            if all(_streams_overlap(o, cands[-1]) for o in others):
                return cands[-1], len(cands)
        import warnings
        warnings.warn("unet_convlstm_amd: no HIP stream runs concurrently with the ones in use; work meant to overlap the "
                      "backward pass will be serialised behind it (try GPU_MAX_HW_QUEUES=8)")
    return (cands[0] if cands else torch.cuda.Stream(device=device)), len(cands)


def side_stream(device) -> "torch.cuda.Stream":
    """The second stream of ``device`` (weight gradients).  Chosen once, at first use, as a stream that runs concurrently
    with the stream current at that moment."""
    key = str(device)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key], _SIDE_STREAM_PROBES[key] = _pick_stream(device, [torch.cuda.current_stream(device)])
    return _SIDE_STREAMS[key]


def launch_stream(device, main: "torch.cuda.Stream") -> "torch.cuda.Stream":
    """A third stream that carries no kernels, only waits: data-parallel code enqueues its collectives from it so that
    neither ``main`` nor the side stream ever blocks on the other.  It must not share a hardware queue with either (a
    wait packet would hold back the kernels queued behind it)."""
    key = str(device)
    if key not in _LAUNCH_STREAMS:
        _LAUNCH_STREAMS[key], _ = _pick_stream(device, [main, side_stream(device)])
    return _LAUNCH_STREAMS[key]


def _schedule_join(device) -> None:
    key = str(device)
    if key in _JOIN_PENDING:
        return
    _JOIN_PENDING.add(key)

    def join():
        _JOIN_PENDING.discard(key)
        torch.cuda.current_stream(device).wait_stream(side_stream(device))

    torch.autograd.Variable._execution_engine.queue_callback(join)


def _on_side(device, launch, keep=()) -> None:
    """``launch()`` with the side stream current, after everything enqueued on the current stream so far.  ``keep``: the tensors
    (or None) it reads, which the caching allocator must not recycle under the side stream.  The caller says where the current
    stream joins again: ``_FWD_SIDE_PENDING`` in a forward pass, ``_schedule_join`` in a backward pass."""
    side = side_stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        launch()
        for t in keep:
            if t is not None:
                t.record_stream(side)


def wgrad_into_param(weight: torch.Tensor, desc: L.PackDesc, inputs: Sequence[torch.Tensor], run_gemm) -> Optional[torch.Tensor]:
    """Weight gradient of one layer.  ``run_gemm()`` launches the weight-gradient GEMM and returns the f32 panel.
    Returns the gradient tensor for autograd, or ``None`` after accumulating into ``weight.grad`` on the side stream."""
    g = weight.grad
    if not (ASYNC_WGRAD and g is not None and g.dtype == F32 and g.is_contiguous() and g.shape == weight.shape):
        return unpack_wgrad(desc, run_gemm(), weight)

    def launch():
        global _WGRAD_OVERLAPPED
        _WGRAD_OVERLAPPED = True
        try:
            dwp = run_gemm()
        finally:
            _WGRAD_OVERLAPPED = False
        _unpack_wgrad_launch(desc, dwp, g, 1)           # (scratch of the ordered form: allocated and freed under the side stream)
        for hook in GRAD_SIDE_HOOKS:
            hook(weight)

    _on_side(weight.device, launch, inputs)
    _schedule_join(weight.device)
    return None


def direct_grad(param: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """``param.grad`` when a backward kernel may accumulate into it directly (pre-attached contiguous f32 buffer, as
    ``optim.FlatParams`` provides), else ``None``.  Saves autograd's tiny per-parameter accumulate kernels."""
    if param is None or not DIRECT_GRADS:
        return None
    g = param.grad
    if g is None or g.dtype != F32 or not g.is_contiguous() or g.shape != param.shape:
        return None
    return g


def direct_grad_pair(weight: torch.Tensor, bias: Optional[torch.Tensor], need_w: bool, need_b: bool):
    """``(weight.grad, bias.grad)`` where ONE kernel that adds into both may write the two gradients directly, else ``None``
    (the kernel then gets scratch buffers and autograd the results).  All or nothing: both trainable and both with an attached
    buffer (``direct_grad``); an absent bias does not stand in the way."""
    if not (need_w and (need_b or bias is None)):
        return None
    gw, gb = direct_grad(weight), direct_grad(bias)
    if gw is None or (bias is not None and gb is None):
        return None
    return gw, gb


def grad_written(param: torch.Tensor) -> None:
    """Tell data-parallel code that ``param.grad`` has been written outside autograd's accumulator."""
    for hook in GRAD_SIDE_HOOKS:
        hook(param)


# A parameter whose gradient is written outside autograd announces itself once per USE (autograd's own accumulator fires
# once per backward pass, however often the parameter was used).  Operators therefore report every use in forward, so that
# a data-parallel wrapper knows how many announcements complete a parameter -- a module called twice before one backward
# (reference-style per-timestep loops over ConvLSTMCell, two forwards under one loss) must not release its bucket early.
USE_HOOKS: list = []


def note_use(*params) -> None:
    if USE_HOOKS:
        for p in params:
            if p is not None:
                for hook in USE_HOOKS:
                    hook(p)


# ---------------------------------------------------------------------------------------------
# raw launches
# ---------------------------------------------------------------------------------------------
# A single GEMM launch addresses every operand through a 32-bit buffer descriptor whose bit 31 means "outside the tensor"
# (that is how padding is free), so one launch sees at most ~2 GiB of each tensor.  The reference, which runs one timestep
# at a time, has no such limit: batched launches over n_img = T*B images are therefore cut into image ranges here -- on
# BatchNorm-group (timestep) boundaries when the launch also produces statistics, whose rows are per group anyway.
LAUNCH_BYTES_LIMIT = (1 << 31) - (1 << 23)


def _img_chunks(n_img: int, groups: int, bytes_per_img: int, what: str, whole_groups: bool = False) -> List[Tuple[int, int]]:
    """Image ranges [i0, i1) of at most LAUNCH_BYTES_LIMIT bytes each; with ``whole_groups`` (the launch writes per-group
    BatchNorm partial sums) a range is a whole number of groups of n_img/groups images."""
    if n_img * bytes_per_img < LAUNCH_BYTES_LIMIT:
        return [(0, n_img)]
    ipg = n_img // groups
    unit = ipg if whole_groups else 1
    per = ((LAUNCH_BYTES_LIMIT - 1) // (bytes_per_img * unit)) * unit
    if per < unit or per == 0:
        raise L.UclstmError(f"{what}: one {'BatchNorm group' if whole_groups else 'image'} of this tensor ({unit} image(s) x "
                            f"{bytes_per_img} bytes) exceeds the {LAUNCH_BYTES_LIMIT}-byte range a single launch can address; "
                            "use a smaller per-GPU batch")
    return [(i, min(n_img, i + per)) for i in range(0, n_img, per)]


def _bytes_per_img(t: torch.Tensor) -> int:
    return t[0].numel() * t.element_size()


def _same_act_dtype(tensors, what: str) -> None:
    dt = tensors[0].dtype
    if dt not in ACT or any(t.dtype != dt for t in tensors):
        raise L.UclstmError(f"{what}: activations, panels and outputs must share one 16-bit dtype, got {[str(t.dtype) for t in tensors]}")


# Split-K for STORE-epilogue convolutions whose tile grid cannot fill the chip (no BatchNorm statistics wanted: inference, or
# evaluation-mode statistics): below SPLITK_STORE_BELOW 128 x 128 tiles.  UCLSTM_SPLITK_STORE=0 switches it off.
SPLITK_STORE = os.environ.get("UCLSTM_SPLITK_STORE", "1") != "0"
SPLITK_STORE_BELOW = int(os.environ.get("UCLSTM_SPLITK_STORE_BELOW", "192"))
# Second rule, OFF by default (UCLSTM_SPLITK_STORE_LONGK=288 switches it on): a grid of 128 x 256 tiles that needs a second round of the
# 256 CUs for at most half a round's worth of tiles, on a LONG K, as two K ranges.  Measured (tools/bench_store_splitk.py,
# profiles/round3_store_splitk.txt, finish pass included): alone, 320 tiles x K = 36864 (the temporal ConvLSTM's input gradient over all
# timesteps) 823 -> 632 us and 384 tiles (the same layer at 256 x 256, B = 4) 792 -> 741 us; 320 tiles x K = 9216 +-3 %; every other
# under-filled shape (160 / 320 / 640 tiles, K <= 18432) LOSES 2 - 70 %.  In the STEP, where the weight-gradient stream runs beside
# the main stream, the rule fires (igemm_fwd_store_splitk, 0.786 -> 0.611 ms serialised) and the backward phase gets no shorter:
# 20.643 -> 20.678 ms, slower in three of three same-box pairs (profiles/round3_store_splitk_step_ab.txt) -- the CUs the under-filled
# round leaves idle are taken by the other stream, and the slabs + finish pass are extra work.  Useful only for serialised /
# single-stream execution, hence a switch and not the default.
SPLITK_STORE_LONGK_STEPS = int(os.environ.get("UCLSTM_SPLITK_STORE_LONGK", "0"))          # K-steps of 64 from which it applies; 0 = off


def store_split_k(pixels: int, N: int, ksteps: int) -> int:
    """K ranges of a store-epilogue convolution without BatchNorm statistics (1 = one pass).  Pure function of the shape."""
    ks = split_k_factor(pixels, N, ksteps, min_blocks=SPLITK_STORE_BELOW)
    if ks == 1 and SPLITK_STORE_LONGK_STEPS > 0 and ksteps >= SPLITK_STORE_LONGK_STEPS:
        tiles = ((pixels + 127) // 128) * ((N + 255) // 256)
        if 256 < tiles <= 384:
            ks = 2
    return ks


def igemm_store(srcs: Sequence[SrcView], wp: torch.Tensor, out_hw: Tuple[int, int], n_img: int, segs, *, ktap: int, scale: int = 1,
                pad: int = 0, groups: int = 1, bias=None, col_scale=None, col_shift=None, relu: bool = False, stats=None) -> None:
    """segs: list of (tensor, n_begin, n_end, c_off, scale, oy, ox).  ``stats``: [groups, tiles_per_group, N, 2]."""
    per_img = max([_bytes_per_img(sv.t) for sv in srcs] + [_bytes_per_img(sg[0]) for sg in segs])
    chunks = _img_chunks(n_img, groups, per_img, "igemm_fwd(store)", whole_groups=stats is not None)
    if len(chunks) > 1:
        if LAUNCH_LOG is not None:
            LAUNCH_LOG.append(("split", "igemm_fwd(store)", len(chunks)))
        ipg = n_img // groups
        for i0, i1 in chunks:
            sub_src = [SrcView(sv.t[i0:i1], sv.offY, sv.offX) for sv in srcs]
            sub_seg = [(sg[0][i0:i1],) + tuple(sg[1:]) for sg in segs]
            sub_stats = None if stats is None else stats[i0 // ipg:i1 // ipg]
            igemm_store(sub_src, wp, out_hw, i1 - i0, sub_seg, ktap=ktap, scale=scale, pad=pad,
                        groups=(i1 - i0) // ipg if stats is not None else 1, bias=bias, col_scale=col_scale, col_shift=col_shift,
                        relu=relu, stats=sub_stats)
        return
    if stats is None and SPLITK_STORE and scale == 1 and len(segs) == 1:
        # few output pixels (batch-1 inference: a 32 x 32 bottleneck is 4 x 8 tiles for 256 CUs): K ranges store f32 partial
        # tiles, uclstm_splitk_finish applies the epilogue.  Only for one dense destination (a plain convolution).
        t, n_begin, n_end, c_off, sg_scale, oy, ox = (tuple(segs[0]) + (0, 1, 0, 0))[:7]
        N, pixels = wp.shape[0], n_img * out_hw[0] * out_hw[1]
        if (n_begin, n_end, c_off, sg_scale, oy, ox) == (0, N, 0, 1, 0, 0) and t.is_contiguous() and tuple(t.shape) == (n_img, out_hw[0], out_hw[1], N):
            ksplit = store_split_k(pixels, N, wp.shape[1] // 64)
            if ksplit > 1:
                nsl = ksplit_used(wp.shape[1], ksplit, ktap)
                pre = torch.empty((nsl, pixels, N), dtype=F32, device=t.device)
                igemm_atomic(srcs, wp, out_hw, n_img, pre, ksplit, ktap=ktap, pad=pad, slabs=True, kind="igemm_fwd_store_splitk")
                L.check(_k(wp).uclstm_splitk_finish(_p(pre), nsl, pre.stride(0), N, _p(bias), _p(col_scale), _p(col_shift), int(relu), _p(t),
                                                    pixels, N, _stream()), "splitk_finish")
                return
    d = L.IgemmDesc()
    d.n_img, d.H, d.W, d.groups = n_img, out_hw[0], out_hw[1], groups
    d.ktap, d.scale, d.pad, d.nsrc = ktap, scale, pad, len(srcs)
    for i, s in enumerate(srcs):
        s.fill(d.src[i])
    d.wp, d.N, d.Ktot = wp.data_ptr(), wp.shape[0], wp.shape[1]
    d.bias = None if bias is None else bias.data_ptr()
    d.col_scale = None if col_scale is None else col_scale.data_ptr()
    d.col_shift = None if col_shift is None else col_shift.data_ptr()
    d.relu, d.epi = int(relu), L.EPI_STORE
    d.nseg = len(segs)
    for i, sg in enumerate(segs):
        _fill_seg(d.seg[i], *sg)
    d.stats = None if stats is None else stats.data_ptr()
    flops = 2.0 * n_img * out_hw[0] * out_hw[1] * d.N * ktap * ktap * sum(s.t.shape[3] for s in srcs)
    _log_shape(d)
    _same_act_dtype([sv.t for sv in srcs] + [wp] + [sg[0] for sg in segs], "igemm_fwd(store)")
    K = _k(wp)
    _timed(_kernel_kind("igemm_fwd_store", d), flops, lambda: L.check(K.uclstm_igemm_fwd(C.byref(d), _stream()), "igemm_fwd(store)"),
           f"M={n_img * out_hw[0] * out_hw[1]} N={d.N} K={d.Ktot} ktap={ktap} nsrc={len(srcs)} nseg={len(segs)}",
           nbytes=_nb(*[sv.t for sv in srcs], wp) + 2.0 * n_img * out_hw[0] * out_hw[1] * d.N if PROFILE is not None else 0.0)


def split_k_factor(pixels: int, N: int, ksteps: int, min_blocks: int = 384, target: int = 512) -> int:
    """K ranges for a GEMM whose 128x128 tile grid alone cannot fill the 256 CUs (the per-timestep GEMMs of the
    ConvLSTM recurrence: M = B*h*w is as small as 512).  1 = do not split."""
    tiles = ((pixels + 127) // 128) * ((N + 127) // 128)
    if tiles >= min_blocks:
        return 1
    return max(1, min((target + tiles - 1) // tiles, ksteps // 8))


def ksplit_used(Ktot: int, ksplit: int, ktap: int = 3) -> int:
    """K ranges the library really uses for a requested split (whole chunks of ktap^2 K-steps, every range non-empty) = slab
    count of ``slabs=True``."""
    n = int(L.lib.uclstm_igemm_ksplit_used(Ktot, ktap, ksplit))
    if n < 1:
        raise L.UclstmError(f"igemm_ksplit_used({Ktot}, {ktap}, {ksplit}): bad argument")
    return n


def _atomic_desc(srcs: Sequence[SrcView], wp: torch.Tensor, out_hw: Tuple[int, int], n_img: int, acc_out: torch.Tensor, ksplit: int, *,
                 ktap: int, scale: int = 1, pad: int = 0, slabs: bool = False):
    """Descriptor of a split-K launch: (desc, algorithmic flops, algorithmic bytes, note, tensors to keep alive)."""
    _dev(acc_out, F32, "acc_out")
    d = L.IgemmDesc()
    d.n_img, d.H, d.W, d.groups = n_img, out_hw[0], out_hw[1], 1
    d.ktap, d.scale, d.pad, d.nsrc = ktap, scale, pad, len(srcs)
    for i, s in enumerate(srcs):
        s.fill(d.src[i])
    d.wp, d.N, d.Ktot = wp.data_ptr(), wp.shape[0], wp.shape[1]
    d.relu, d.epi, d.nseg = 0, L.EPI_ATOMIC, 0
    d.acc_out, d.acc_ld, d.ksplit = acc_out.data_ptr(), acc_out.shape[-1], ksplit
    d.acc_slab = acc_out.stride(0) if slabs else 0
    if slabs and (acc_out.dim() != 3 or acc_out.shape[0] != ksplit_used(d.Ktot, ksplit, ktap) or not acc_out.is_contiguous()):
        raise L.UclstmError("igemm_atomic(slabs=True): acc_out must be a contiguous [ksplit_used, pixels, ld] tensor")
    flops = 2.0 * n_img * out_hw[0] * out_hw[1] * d.N * ktap * ktap * sum(s.t.shape[3] for s in srcs)
    _same_act_dtype([sv.t for sv in srcs] + [wp], "igemm_fwd(atomic)")
    nbytes = _nb(*[sv.t for sv in srcs], wp) + 4.0 * n_img * out_hw[0] * out_hw[1] * d.N if PROFILE is not None else 0.0
    return d, flops, nbytes, f"M={n_img * out_hw[0] * out_hw[1]} N={d.N} K={d.Ktot} ktap={ktap} ksplit={ksplit}"


def igemm_atomic(srcs: Sequence[SrcView], wp: torch.Tensor, out_hw: Tuple[int, int], n_img: int, acc_out: torch.Tensor, ksplit: int, *,
                 ktap: int, scale: int = 1, pad: int = 0, slabs: bool = False, kind: str = "igemm_fwd_atomic") -> None:
    """Split-K convolution as `ksplit` K ranges.  ``slabs=False``: acc_out[pixel, n] += ... with f32 atomics
    (acc_out f32 [pixels, ld>=N], zeroed by the caller).  ``slabs=True``: acc_out is [ksplit_used, pixels, ld]; range r
    stores into acc_out[r] and the consumer adds the slabs (plain stores run ~4.6x faster than float atomics)."""
    _igemm_launch(_atomic_desc(srcs, wp, out_hw, n_img, acc_out, ksplit, ktap=ktap, scale=scale, pad=pad, slabs=slabs), _k(wp), kind,
                  "igemm_fwd(atomic)")


def _igemm_launch(item, K, kind: str, what: str) -> None:
    """One uclstm_igemm_fwd launch of a (desc, flops, nbytes, note) item of _atomic_desc / _lstm_desc."""
    d, flops, nbytes, note = item
    _log_shape(d)
    _timed(_kernel_kind(kind, d), flops, lambda: L.check(K.uclstm_igemm_fwd(C.byref(d), _stream()), what), note, nbytes=nbytes)


def _lstm_desc(x: Optional[torch.Tensor], h_prev: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], c_prev: Optional[torch.Tensor],
               c_out: Optional[torch.Tensor], h_out: Optional[torch.Tensor], gates_out: Optional[torch.Tensor], ksize: int = 3,
               pre_add: Optional[torch.Tensor] = None, probe: Optional[tuple] = None):
    """Descriptor of a fused ConvLSTM cell step, as (desc, flops, nbytes, note).  ``probe`` = (B, H, W, source channel counts, N, Ktot,
    placeholder pointer) instead of the tensors: the same descriptor for the library's planners, which read the shapes and
    dereference no pointer."""
    d = L.IgemmDesc()
    if probe is not None:
        B, H, W, chans, d.N, d.Ktot, ptr = probe
        d.nsrc = len(chans)
        for i, cch in enumerate(chans):
            d.src[i].ptr, d.src[i].C, d.src[i].Hs, d.src[i].Ws = ptr, cch, H, W
        d.wp = d.c_out = d.h_out = ptr
    else:
        B, H, W, _ = h_prev.shape
        srcs = [h_prev] if x is None else [x, h_prev]
        d.nsrc = len(srcs)
        for i, t in enumerate(srcs):
            SrcView(t).fill(d.src[i])
        d.wp, d.N, d.Ktot = wp.data_ptr(), wp.shape[0], wp.shape[1]
        d.c_out, d.h_out = c_out.data_ptr(), h_out.data_ptr()
    d.n_img, d.H, d.W, d.groups = B, H, W, 1
    d.ktap, d.scale, d.pad = ksize, 1, ksize // 2
    d.relu, d.epi, d.nseg = 0, L.EPI_LSTM, 0
    d.Hd_p = d.src[d.nsrc - 1].C
    if probe is not None:
        return d, 0.0, 0.0, "probe"
    d.pre_add = None if pre_add is None else _dev(pre_add, F32, "pre_add").data_ptr()
    d.bias = None if bias is None else bias.data_ptr()
    d.c_prev = None if c_prev is None else c_prev.data_ptr()
    d.gates_out = None if gates_out is None else gates_out.data_ptr()
    flops = 2.0 * B * H * W * (4 * d.Hd_p) * ksize * ksize * ((x.shape[3] if x is not None else 0) + h_prev.shape[3])
    _same_act_dtype([h_prev, wp, h_out] + ([x] if x is not None else []) + ([gates_out] if gates_out is not None else []), "igemm_fwd(lstm)")
    nbytes = _nb(x, h_prev, wp, c_prev, c_out, h_out, gates_out, pre_add) if PROFILE is not None else 0.0
    return d, flops, nbytes, f"M={B * H * W} N={d.N} K={d.Ktot}"


def igemm_lstm(x: Optional[torch.Tensor], h_prev: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], c_prev: Optional[torch.Tensor],
               c_out: torch.Tensor, h_out: torch.Tensor, gates_out: Optional[torch.Tensor], ksize: int = 3,
               pre_add: Optional[torch.Tensor] = None) -> None:
    """Fused ConvLSTM cell step.  ``x`` given: gate conv over (x_t, h_{t-1}) with the two-source panel.  ``x=None``: the
    launch carries W_h * h_{t-1} only and ``pre_add`` (f32 [pixels, N]) holds the hoisted W_x * x_t."""
    _igemm_launch(_lstm_desc(x, h_prev, wp, bias, c_prev, c_out, h_out, gates_out, ksize, pre_add), _k(wp), "igemm_fwd_lstm", "igemm_fwd(lstm)")


def igemm_group(items, K, kind: str = "igemm_fwd_group", tap: bool = False) -> None:
    """``items``: [(desc, flops, nbytes, note)] of INDEPENDENT launches -> one uclstm_igemm_fwd_group launch (``tap``: one
    uclstm_igemm_fwd_group_tap launch, the group of the 128 x 128 per-tap shape)."""
    arr = (L.IgemmDesc * len(items))(*[it[0] for it in items])
    for it in items:
        _log_shape(it[0])
    entry, what, shape = (K.uclstm_igemm_fwd_group_tap, "igemm_fwd_group_tap", "[pertap128x128]") if tap else \
                         (K.uclstm_igemm_fwd_group, "igemm_fwd_group", "[patch128x256]")
    _timed(kind + shape if PROFILE is not None else kind, sum(it[1] for it in items),
           lambda: L.check(entry(arr, len(items), _stream()), what),
           " | ".join(it[3] for it in items), nbytes=sum(it[2] for it in items))


def group_launchable(descs) -> bool:
    """True when uclstm_igemm_fwd_group accepts these descriptors as one launch (all on the patch shape, same source count)."""
    arr = (L.IgemmDesc * len(descs))(*descs)
    return int(L.lib.uclstm_igemm_fwd_group_blocks(arr, len(descs))) > 0


def igemm_wgrad(srcs: Sequence[SrcView], dy_segs, N: int, Ktot: int, out_hw: Tuple[int, int], n_img: int, *, ktap: int, scale: int = 1,
                pad: int = 0) -> torch.Tensor:
    """Weight-gradient GEMM; returns the f32 panel gradient as pixel-range slabs [splits, N, Ktot] (the unpack adds them).
    Operands beyond the single-launch byte range are processed as image ranges, each range contributing its own slabs."""
    dev = srcs[0].t.device
    _same_act_dtype([sv.t for sv in srcs] + [sg[0] for sg in dy_segs], "igemm_wgrad")
    K = _k(srcs[0].t)
    per_img = max([_bytes_per_img(sv.t) for sv in srcs] + [_bytes_per_img(sg[0]) for sg in dy_segs])
    chunks = _img_chunks(n_img, 1, per_img, "igemm_wgrad")
    descs = []
    for i0, i1 in chunks:
        d = L.WgradDesc()
        d.n_img, d.H, d.W = i1 - i0, out_hw[0], out_hw[1]
        d.ktap, d.scale, d.pad, d.nsrc = ktap, scale, pad, len(srcs)
        for i, sv in enumerate(srcs):
            (sv if len(chunks) == 1 else SrcView(sv.t[i0:i1], sv.offY, sv.offX)).fill(d.src[i])
        d.N, d.Ktot = N, Ktot
        d.nseg = len(dy_segs)
        for i, sg in enumerate(dy_segs):
            _fill_seg(d.seg[i], *(sg if len(chunks) == 1 else (sg[0][i0:i1],) + tuple(sg[1:])))
        # slab mode: every pixel range stores its partial panel into its own slab (no float atomics, nothing to zero);
        # the library picks the range count for its tile shape and the 256 CUs, uclstm_unpack_wgrad adds the slabs
        d.splits, d.accumulate, d.slab = 0, 1, N * Ktot
        d.overlapped = int(_WGRAD_OVERLAPPED)          # on the side stream: the plan that interferes least with the main stream
        splits = int(L.lib.uclstm_igemm_wgrad_splits(C.byref(d)))
        if splits < 1:
            raise L.UclstmError(f"igemm_wgrad: bad descriptor (code {splits})")
        d.splits = splits
        descs.append(d)
    if LAUNCH_LOG is not None:
        if len(chunks) > 1:
            LAUNCH_LOG.append(("split", "igemm_wgrad", len(chunks)))
        for d in descs:
            LAUNCH_LOG.append(("wgrad", int(L.lib.uclstm_igemm_wgrad_shape(C.byref(d))), N, Ktot, int(d.splits)))
    total = sum(d.splits for d in descs)
    dwp = torch.empty((total, N, Ktot), dtype=F32, device=dev)
    taps = ktap * ktap
    at = 0
    for d in descs:
        d.dwp = dwp[at].data_ptr()
        at += d.splits
        flops = 2.0 * d.n_img * out_hw[0] * out_hw[1] * N * taps * sum(s.t.shape[3] for s in srcs)
        kind = "igemm_wgrad"
        if PROFILE is not None:          # rocprofv3 names: igemm_wgrad_p3_kernel / igemm_wgrad_p2_kernel<1 or 2, nsrc> / igemm_wgrad_kernel
            kind += "[" + {4: "ring64", 3: "p3_256x256", 2: "p2_128x128", 1: "p2_64x256", 0: "generic"}.get(int(L.lib.uclstm_igemm_wgrad_shape(C.byref(d))), "?") + "]"
        _timed(kind, flops, lambda d=d: L.check(K.uclstm_igemm_wgrad(C.byref(d), _stream()), "igemm_wgrad"),
               f"M={d.n_img * out_hw[0] * out_hw[1]} N={N} K={Ktot} ktap={ktap} splits={d.splits}",
               nbytes=(_nb(*[sv.t for sv in srcs], *[sg[0] for sg in dy_segs]) * (d.n_img / n_img) + 4.0 * N * Ktot) if PROFILE is not None else 0.0)
    return dwp


def colsum(a: torch.Tensor, into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Column sums of a 16-bit [pixels, Cp] tensor.  ``into``: f32 [Cp] buffer the sums are ADDED to (e.g. an attached bias
    gradient: saves the zero-fill, the slice copy and autograd's accumulate kernel); else a fresh zeroed vector."""
    _dev(a, ACT, "colsum input")
    Cp = a.shape[-1]
    if _DETERMINISTIC:
        pixels = a.numel() // Cp
        out = into if into is not None else torch.empty((Cp,), dtype=F32, device=a.device)
        partials = torch.empty((int(L.lib.uclstm_colsum_ordered_rows(pixels, Cp)), Cp), dtype=F32, device=a.device)
        _log_reduce("colsum_ordered")
        L.check(L.lib.uclstm_colsum_ordered(_p(a), _p(partials), _p(out), pixels, Cp, 1 if into is not None else 0, L.act_type(a.dtype),
                                            _stream()), "colsum_ordered")
        return out
    out = into if into is not None else torch.zeros((Cp,), dtype=F32, device=a.device)
    _log_reduce("colsum")
    L.check(_k(a).uclstm_colsum(_p(a), _p(out), a.numel() // Cp, Cp, _stream()), "colsum")
    return out


def bias_grad_from_colsum(a: torch.Tensor, bias: Optional[torch.Tensor], valid: int) -> Optional[torch.Tensor]:
    """Bias gradient = column sums of ``a`` ([..., Cp], ``valid`` real channels).  When the bias owns an attached f32 gradient
    of exactly Cp elements the kernel accumulates straight into it and ``None`` is returned for autograd."""
    if bias is None:
        return None
    g = direct_grad(bias)
    if g is not None and g.numel() == a.shape[-1] == valid:
        # (moving this HBM-bound pass to the weight-gradient stream was measured: no gain, unlike the tiny BatchNorm
        # parameter-gradient kernels below)
        colsum(a, into=g.view(-1))
        grad_written(bias)
        return None
    return colsum(a)[:valid].contiguous()


# ---------------------------------------------------------------------------------------------
# layout conversion at the module boundary
# ---------------------------------------------------------------------------------------------
class ToNHWC(torch.autograd.Function):
    """f32 NCHW [N,C,H,W] -> bf16 NHWC [N,H,W,Cp]."""

    @staticmethod
    def forward(ctx, x):
        _dev(x, F32, "input")
        N, Cc, H, W = x.shape
        out = torch.empty((N, H, W, cpad(Cc)), dtype=_COMPUTE_DTYPE, device=x.device)
        L.check(_k(out).uclstm_nchw_to_nhwc(_p(x), _p(out), N, Cc, cpad(Cc), H, W, N, 0, Cc * H * W, _stream()), "nchw_to_nhwc")
        ctx.C = Cc
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, H, W, Cp = g.shape
        out = torch.empty((N, ctx.C, H, W), dtype=F32, device=g.device)
        L.check(_k(g).uclstm_nhwc_to_nchw(_p(g), _p(out), N, ctx.C, Cp, H, W, _stream()), "nhwc_to_nchw")
        return out


class FromNHWC(torch.autograd.Function):
    """bf16 NHWC [N,H,W,Cp] -> f32 NCHW [N,C,H,W]."""

    @staticmethod
    def forward(ctx, a, Cc):
        _dev(a, ACT, "activation")
        N, H, W, Cp = a.shape
        out = torch.empty((N, Cc, H, W), dtype=F32, device=a.device)
        L.check(_k(a).uclstm_nhwc_to_nchw(_p(a), _p(out), N, Cc, Cp, H, W, _stream()), "nhwc_to_nchw")
        ctx.Cp = Cp
        ctx.act_dtype = a.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, Cc, H, W = g.shape
        out = torch.empty((N, H, W, ctx.Cp), dtype=ctx.act_dtype, device=g.device)
        L.check(_k(out).uclstm_nchw_grad_to_nhwc(_p(g), _p(out), N, Cc, ctx.Cp, H, W, _stream()), "nchw_grad_to_nhwc")
        return out, None


class StateToNHWC(torch.autograd.Function):
    """f32 NCHW cell state -> f32 NHWC [N,H,W,Cp]."""

    @staticmethod
    def forward(ctx, c):
        _dev(c, F32, "cell state")
        N, Cc, H, W = c.shape
        out = torch.empty((N, H, W, cpad(Cc)), dtype=F32, device=c.device)
        L.check(L.lib.uclstm_nchw_to_nhwc_f32(_p(c), _p(out), N, Cc, cpad(Cc), H, W, _stream()), "nchw_to_nhwc_f32")
        ctx.C = Cc
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, H, W, Cp = g.shape
        out = torch.empty((N, ctx.C, H, W), dtype=F32, device=g.device)
        L.check(L.lib.uclstm_nhwc_to_nchw_f32(_p(g), _p(out), N, ctx.C, Cp, H, W, _stream()), "nhwc_to_nchw_f32")
        return out


class StateFromNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c, Cc):
        _dev(c, F32, "cell state")
        N, H, W, Cp = c.shape
        out = torch.empty((N, Cc, H, W), dtype=F32, device=c.device)
        L.check(L.lib.uclstm_nhwc_to_nchw_f32(_p(c), _p(out), N, Cc, Cp, H, W, _stream()), "nhwc_to_nchw_f32")
        ctx.Cp = Cp
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, Cc, H, W = g.shape
        out = torch.empty((N, H, W, ctx.Cp), dtype=F32, device=g.device)
        L.check(L.lib.uclstm_nchw_to_nhwc_f32(_p(g), _p(out), N, Cc, ctx.Cp, H, W, _stream()), "nchw_to_nhwc_f32")
        return out, None


def im2col_first(x: torch.Tensor, time_major: bool) -> torch.Tensor:
    """First-layer gather of a f32 input that needs no gradient.

    ``x`` is ``[N,C,H,W]`` or, with ``time_major``, ``[B,T,C,H,W]`` read as image ``t*B+b``
    (train/unet.py:180 feeds ``x_seq[:, t]``).  Returns bf16 ``[N,H,W,Kp]`` with K = (tap, c).
    """
    _dev(x, F32, "input")
    if time_major:
        B, T, Cc, H, W = x.shape
        n_img, inner, inner_stride, outer_stride = B * T, B, Cc * H * W, T * Cc * H * W
    else:
        n_img, Cc, H, W = x.shape
        inner, inner_stride, outer_stride = n_img, 0, Cc * H * W
    Kp = cpad(9 * Cc)
    out = torch.empty((n_img, H, W, Kp), dtype=_COMPUTE_DTYPE, device=x.device)
    L.check(_k(out).uclstm_im2col3x3_first(_p(x), _p(out), n_img, Cc, Kp, H, W, inner, inner_stride, outer_stride, _stream()),
            "im2col3x3_first")
    return out


# ---------------------------------------------------------------------------------------------
# conv3x3 (+ optional second source) + BatchNorm + ReLU   (train/unet.py:70-71, :98)
# ---------------------------------------------------------------------------------------------
def _eval_bn_constants(gamma, beta, running_mean, running_var, eps, momentum, Co, Cop) -> torch.Tensor:
    """[2, 1, Cop] f32 (scale, shift) of an evaluation-mode BatchNorm, folded into the conv epilogue.  Constants of frozen
    weights: kept in the current PanelCache (StreamingPredictor) like the packed panels, so a rollout frame does not rebuild them."""
    cache, key, ver = _ACTIVE_CACHE, None, None
    if cache is not None and not cache.stale():
        key = ("bn_eval", gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), float(eps), Cop)
        ver = (gamma._version, beta._version, running_mean._version, running_var._version)
        hit = cache.entries.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
    par = torch.empty((2, 1, Cop), dtype=F32, device=gamma.device)
    L.check(L.lib.uclstm_bn_finalize(None, 1, 0, Cop, Co, 0, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                     momentum, eps, _p(par[0]), _p(par[1]), None, None, _stream()), "bn_finalize(eval)")
    if key is not None:
        cache.entries[key] = (ver, par)
    return par


_OUTER_GRAD = True


class _GradAwareFunction(torch.autograd.Function):
    """Function.forward runs with grad mode off and ctx.needs_input_grad ignores torch.no_grad(): remember the CALLER's grad
    mode, so that a forward under no_grad (validation, StreamingPredictor) takes the inference kernels, saves nothing and does
    not count as a use for the data-parallel bucket bookkeeping."""

    @classmethod
    def apply(cls, *args, **kwargs):
        global _OUTER_GRAD
        prev, _OUTER_GRAD = _OUTER_GRAD, torch.is_grad_enabled()
        try:
            return super(_GradAwareFunction, cls).apply(*args, **kwargs)
        finally:
            _OUTER_GRAD = prev


def _will_backward(ctx) -> bool:
    return _OUTER_GRAD and any(ctx.needs_input_grad)


def conv_geometry(x0, x1, weight, c_valid, off, im2col=None, stride: int = 1):
    """(pack descriptor, sources, ktap, scale, pad, Ho, Wo) of a convolution in front of a BatchNorm, of either model, for the
    forward GEMM and the weight gradient alike.  ``im2col``: ``x0`` is a pre-gathered first-layer matrix, a plain GEMM per pixel
    whose panel descriptor ``im2col(Co, Ci, Kp)`` builds; otherwise k x k taps with pad k // 2 over the output grid and one or two
    sources, stride 2 as ``scale = 2`` (k = 1: pad 0 on the same grid).  A plain tuple: the eager frame-by-frame path is host-bound."""
    _, Hs, Ws, Cxp = x0.shape
    Co, Ci_total, k = weight.shape[0], weight.shape[1], weight.shape[2]
    if im2col is not None:
        return im2col(Co, Ci_total, Cxp), [SrcView(x0)], 1, 1, 0, Hs, Ws
    Ho, Wo = (Hs - 1) // stride + 1, (Ws - 1) // stride + 1
    if x1 is None:
        return conv_pack_desc(Co, Ci_total, c_valid, (Cxp,), k), [SrcView(x0)], k, stride, k // 2, Ho, Wo
    return conv_pack_desc(Co, Ci_total, c_valid, (Cxp, x1.shape[3]), k), [SrcView(x0), SrcView(x1, off[0], off[1])], k, stride, k // 2, Ho, Wo


def _bn_forward_stats(stats, n_img, H, W, groups, Co, gamma, beta, running_mean, running_var, momentum, eps, variant):
    """From the convolution's partial sums ``stats`` [groups, tiles, Cop, 2] to ``par`` = (scale, shift, mean, rstd), each
    [groups, Cop], and the running-statistics update.  ``stats`` None: frozen statistics, par from the running ones.
    Returns (par, sync): sync = (process group, world size) where the statistics are those of all ranks (the sync_batchnorm
    switch; ``variant`` goes to LAUNCH_LOG), else None."""
    Cop = cpad(Co)
    par = torch.empty((4, groups, Cop), dtype=F32, device=gamma.device)
    pp = (_p(par[0]), _p(par[1]), _p(par[2]), _p(par[3]))
    if stats is None:
        L.check(L.lib.uclstm_bn_finalize(None, 1, 0, Cop, Co, 0, _p(gamma), _p(beta), _p(running_mean), _p(running_var), momentum, eps,
                                         *pp, _stream()), "bn_finalize(eval)")
        return par, None
    tpg, ppg = stats.shape[1], (n_img // groups) * H * W
    sync, count, on_side = None, ppg, ASYNC_WGRAD and BN_RUNNING_ON_SIDE
    if _SYNC_BN:
        # statistics over all ranks: f64 sums of this rank -> all-reduce -> scale / shift / mean / rstd from the sums of
        # all ranks.  `stats` then holds (mean, variance) of the global batch in its tile-0 slots, and the running
        # statistics below are updated from them with the global count.
        if torch.cuda.is_current_stream_capturing():
            raise L.UclstmError("sync_batchnorm: a step with collectives cannot be captured in a HIP graph")
        world = _sync_bn_check_equal(_SYNC_BN_GROUP, n_img, H, W, groups)
        sync, count = (_SYNC_BN_GROUP, world), world * ppg
        sums64 = torch.empty((groups, Cop, 2), dtype=torch.float64, device=gamma.device)
        if LAUNCH_LOG is not None:
            LAUNCH_LOG.append(("syncbn", "bn_stats_partial", variant))
        L.check(L.lib.uclstm_bn_stats_partial(_p(stats), groups, tpg, Cop, _p(sums64), _stream()), "bn_stats_partial")
        _sync_bn_all_reduce(sums64, _SYNC_BN_GROUP, "bn_stats")
        if LAUNCH_LOG is not None:
            LAUNCH_LOG.append(("syncbn", "bn_stats_from_sums", variant))
        L.check(L.lib.uclstm_bn_stats_from_sums(_p(sums64), count, _p(stats), groups, tpg, Cop, Co, _p(gamma), _p(beta), eps, *pp, _stream()),
                "bn_stats_from_sums")
    elif on_side and not torch.cuda.is_current_stream_capturing():
        # critical part in one launch (reduction + scale / shift / mean / rstd); the in-order running-statistics recursion,
        # which nothing in this step waits for, on the second stream (joined at the end of the forward pass: join_forward_side)
        L.check(L.lib.uclstm_bn_stats_fwd(_p(stats), groups, tpg, Cop, Co, ppg, _p(gamma), _p(beta), eps, *pp, _stream()), "bn_stats_fwd")
    else:
        L.check(L.lib.uclstm_bn_finalize(_p(stats), groups, tpg, Cop, Co, ppg, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                         momentum, eps, *pp, _stream()), "bn_finalize")
        return par, None

    def running_stats():          # the one-launch route's counterpart: the same momentum steps
        L.check(L.lib.uclstm_bn_running_stats(_p(stats), groups, tpg, Cop, Co, count, _p(running_mean), _p(running_var), momentum,
                                              _stream()), "bn_running_stats")

    if on_side:
        _on_side(gamma.device, running_stats, (stats,))
        _FWD_SIDE_PENDING.add(str(gamma.device))
    else:
        running_stats()
    return par, sync


def bn_param_grads(need_gamma: bool, need_beta: bool, gamma, beta, sums, Co: int):
    """(dgamma, dbeta, direct) of one BatchNorm from ``sums`` (sum g, sum g*xhat) [groups, Cop, 2].  ``direct``: both are wanted and
    both own an attached gradient buffer -- one kernel then adds the groups straight into the buffers (instead of sum + 2 copies +
    2 accumulates) and nothing is returned to autograd.  Nothing in the backward pass waits for it: with the weight-gradient
    stream in use it goes there (small dependent launches off the main stream; joined with the weight gradients at the end of
    backward).  Otherwise the wanted ones are returned (one group: its row as it is, no sum launch); nothing is launched for a
    frozen pair (requires_grad False: gamma and beta are independent of each other)."""
    g_gamma, g_beta = direct_grad(gamma), direct_grad(beta)
    if need_gamma and need_beta and g_gamma is not None and g_beta is not None:
        def launch():
            L.check(L.lib.uclstm_bn_bwd_param_grads(_p(sums), sums.shape[0], sums.shape[1], Co, _p(g_gamma), _p(g_beta), 1, _stream()),
                    "bn_bwd_param_grads")
            grad_written(gamma)
            grad_written(beta)

        if ASYNC_WGRAD and PARAM_GRADS_ON_SIDE:
            _on_side(sums.device, launch, (sums,))
            _schedule_join(sums.device)
        else:
            launch()
        return None, None, True
    if not (need_gamma or need_beta):
        return None, None, False
    tot = sums[0] if sums.shape[0] == 1 else sums.sum(dim=0)
    return (tot[:Co, 1].contiguous() if need_gamma else None), (tot[:Co, 0].contiguous() if need_beta else None), False


# The bodies under the autograd Functions of BOTH models -- ConvBNReLU here (TemporalUNetDualView, the decoder of
# PretrainedTemporalUNet) and resnet.EncConv / resnet.BnRelu (its encoder, which also calls them without autograd): plain functions
# on the tuple of conv_geometry and on ``bn`` = (gamma, beta, running mean, running variance, uses batch statistics, momentum
# argument, eps).  The arithmetic of conv + BatchNorm + ReLU, forward and backward, is written here once.
def conv_bn_stats(x0, weight, bias, geom, bn, groups: int = 1, variant: str = "plain"):
    """(z, par, sync): the convolution's pre-BatchNorm output, (scale, shift, mean, rstd) [4, groups, Cop] -- of the batch, with the
    running statistics updated, or (evaluation statistics with a backward pass; ``groups`` 1) of the running statistics -- and
    _bn_forward_stats' marker that the statistics are those of all ranks, which the backward pass must get back."""
    pd, srcs, ktap, scale, pad, Ho, Wo = geom
    gamma, beta, rm, rv, training, mom, eps = bn
    n, Co, dev = x0.shape[0], weight.shape[0], x0.device
    Cop = cpad(Co)
    wp = pack_weights(pd, weight, 0, x0.dtype)
    bp = pack_bias(pd, bias) if bias is not None else None
    z = torch.empty((n, Ho, Wo, Cop), dtype=x0.dtype, device=dev)
    stats = None
    if training:
        stats = torch.empty((groups, L.lib.uclstm_igemm_tiles_per_group(n, Ho, Wo, groups, Cop), Cop, 2), dtype=F32, device=dev)
    else:
        join_forward_side(dev)
    igemm_store(srcs, wp, (Ho, Wo), n, [(z, 0, Cop, 0, 1, 0, 0)], ktap=ktap, scale=scale, pad=pad, groups=groups, bias=bp, stats=stats)
    par, sync = _bn_forward_stats(stats, n, Ho, Wo, groups, Co, gamma, beta, rm, rv, mom, eps, variant)
    return z, par, sync


def conv_bn_fold(x0, weight, bias, geom, bn, relu: bool) -> torch.Tensor:
    """Evaluation statistics without a backward pass: ``bn(conv(x))`` (and ReLU) with BatchNorm's scale and shift in the GEMM's
    epilogue -- one rounding to 16 bits, where ``conv_bn_stats`` + ``bn_relu`` make two."""
    pd, srcs, ktap, scale, pad, Ho, Wo = geom
    gamma, beta, rm, rv, _, mom, eps = bn
    n, Co, dev = x0.shape[0], weight.shape[0], x0.device
    Cop = cpad(Co)
    wp = pack_weights(pd, weight, 0, x0.dtype)
    bp = pack_bias(pd, bias) if bias is not None else None
    out = torch.empty((n, Ho, Wo, Cop), dtype=x0.dtype, device=dev)
    join_forward_side(dev)
    par = _eval_bn_constants(gamma, beta, rm, rv, eps, mom, Co, Cop)
    igemm_store(srcs, wp, (Ho, Wo), n, [(out, 0, Cop, 0, 1, 0, 0)], ktap=ktap, scale=scale, pad=pad, bias=bp, col_scale=par[0],
                col_shift=par[1], relu=relu)
    return out


def bn_relu(z: torch.Tensor, par: torch.Tensor, groups: int = 1) -> torch.Tensor:
    """``relu(z*scale + shift)`` with the constants ``par`` of ``conv_bn_stats``, per group of images."""
    a = torch.empty_like(z)
    Cp = z.shape[-1]
    pixels = z.numel() // Cp
    ppg = (z.shape[0] // groups) * (pixels // z.shape[0])
    _timed_hbm("bn_apply_relu", 4.0 * z.numel(),        # 2 B read + 2 B written per element
               lambda: L.check(_k(z).uclstm_bn_apply_relu(_p(z), _p(a), _p(par[0]), _p(par[1]), pixels, ppg, Cp, _stream()), "bn_apply_relu"))
    return a


def bn_relu_backward(z, par, da, groups: int, training: bool, sync, want_dz: bool = True, want_sums: bool = True, sums=None):
    """(dz, sums) of ``bn_relu``: uclstm_bn_bwd_reduce for the per-group sums (sum g, sum g*xhat) [groups, Cp, 2] -- dbeta and
    dgamma -- and uclstm_bn_bwd_apply for the gradient of the conv output; either is None, and its kernel not launched, where the
    caller wants it not (batch statistics: ``dz`` needs the sums; ``sums``: those of an earlier call, for a caller that launches
    something between the two kernels).  Training: dz = scale*(g - s1/n - xhat*s2/n), with the sums of all ranks where the forward
    pass had their statistics (``sync`` of conv_bn_stats).  Evaluation-mode statistics are constants, the two mean terms vanish:
    the same kernel with zero sums gives dz = scale*g (``sums`` itself still holds dbeta / dgamma)."""
    Cp, dev = z.shape[-1], z.device
    pixels = z.numel() // Cp
    ppg = (z.shape[0] // groups) * (pixels // z.shape[0])
    K, da = _k(z), da.contiguous()
    pq = (_p(par[0]), _p(par[1]), _p(par[2]), _p(par[3]))
    dz = None
    if want_sums:
        sums = torch.empty((groups, Cp, 2), dtype=F32, device=dev)
        partials = torch.empty((int(L.lib.uclstm_bn_bwd_reduce_rows(pixels, ppg)), Cp, 2), dtype=F32, device=dev)
        _timed_hbm("bn_bwd_reduce", 4.0 * z.numel(),            # z and da read once
                   lambda: L.check(K.uclstm_bn_bwd_reduce(_p(z), _p(da), *pq, _p(partials), _p(sums), pixels, ppg, Cp, _stream()),
                                   "bn_bwd_reduce"))
    if want_dz:
        dz = torch.empty_like(z)
        if sync is not None:
            sums_dz = _bn_bwd_sums_over_ranks(sums, sync, "plain")
        else:
            sums_dz = sums if training else torch.zeros((groups, Cp, 2), dtype=F32, device=dev)
        _timed_hbm("bn_bwd_apply", 6.0 * z.numel(),             # z, da read, dz written
                   lambda: L.check(K.uclstm_bn_bwd_apply(_p(z), _p(da), *pq, _p(sums_dz), _p(dz), pixels, ppg, Cp, _stream()), "bn_bwd_apply"))
    return dz, sums


def conv_wgrad(weight, geom, dz):
    """Weight gradient of the convolution of ``geom`` from the gradient ``dz`` of its output, through wgrad_into_param."""
    pd, srcs, ktap, scale, pad, Ho, Wo = geom
    n, Cop = dz.shape[0], dz.shape[3]
    return wgrad_into_param(weight, pd, [s.t for s in srcs] + [dz],
                            lambda: igemm_wgrad(srcs, [(dz, 0, Cop, 0, 1, 0, 0)], pd.N, pd.Ktot, (Ho, Wo), n, ktap=ktap, scale=scale, pad=pad))


def conv3x3_dgrad(dz, weight, like, c_valid_s: int, elem_offset: int = 0, oy: int = 0, ox: int = 0) -> torch.Tensor:
    """Input gradient of a conv3x3 / stride 1 / pad 1 for ONE source, shaped as ``like``: the source whose ``c_valid_s`` channels
    start ``elem_offset`` f32 elements into ``weight`` and which was placed at (-oy, -ox) in the output frame."""
    dd = conv_dgrad_pack_desc(weight.shape[0], weight.shape[1], c_valid_s)
    wd = pack_weights(dd, weight, elem_offset, dz.dtype)
    dx = torch.empty_like(like)
    igemm_store([SrcView(dz)], wd, (dz.shape[1], dz.shape[2]), dz.shape[0], [(dx, 0, dd.N, 0, 1, oy, ox)], ktap=3, pad=1)
    return dx


class ConvBNReLU(_GradAwareFunction):
    """One (conv3x3 pad 1 + bias -> BatchNorm2d -> ReLU) stage on NHWC bf16.

    ``x1`` (optional) is channel-concatenated after ``x0`` and may be smaller, centred by
    ``(offY, offX)`` (the F.pad of train/unet.py:95-97).  ``groups`` = number of BatchNorm
    statistic groups along the image axis (timesteps).  ``im2col=True`` means ``x0`` is the
    pre-gathered first-layer tensor (K = 9*Cin) and the conv runs as a plain GEMM.
    """

    @staticmethod
    def forward(ctx, x0, x1, weight, bias, gamma, beta, running_mean, running_var, c_valid, off, groups, training, momentum, eps,
                im2col, head_w=None, head_b=None, pool=False):
        # pool: also return MaxPool2d(2) of the activation -- (a, p) -- with the pooling fused into the BatchNorm kernels both ways
        # (uclstm_bn_apply_relu_pool / uclstm_bn_pool_bwd_*); every encoder block output feeds the next block's pooling and a skip.
        # head_w / head_b: the model's 1x1 output convolution (ONE output channel) fused into this stage (training mode only,
        # uclstm_bn_head_*): the stage then returns y f32 [n_img, 1, H, W] instead of its activation, which never exists.
        _dev(x0, ACT, "x0")
        Co, Ci_total, Cop = weight.shape[0], weight.shape[1], cpad(weight.shape[0])
        (n_img, H, W, _), dev = x0.shape, x0.device
        if head_w is not None and not training:
            raise L.UclstmError("ConvBNReLU: the fused output head is a training-mode path")
        # which BatchNorm kernels the stage takes, decided here once: the fused head, the fused pooling (training mode, even
        # sizes, at most 256 channel chunks per pixel: uclstm_bn_pool_bwd_rows refuses more) or the plain ones
        variant = "head" if head_w is not None else \
            "pool" if (pool and training and H % 2 == 0 and W % 2 == 0 and Cop // 8 <= 256) else "plain"
        geom = conv_geometry(x0, x1, weight, c_valid, off, im2col_pack_desc if im2col else None)
        bn = (gamma, beta, running_mean, running_var, training, momentum, eps)
        K = _k(x0)
        need_bw = _will_backward(ctx)
        pooled = sync = None            # sync: (process group, world size) where this stage's statistics are those of all ranks
        if training or need_bw:
            if not training:
                # evaluation-mode statistics WITH a backward pass (fine-tuning through frozen BatchNorm): keep the pre-BN conv
                # output like the training path does, normalise with the running statistics as one group
                groups = 1
            pixels, ppg = n_img * H * W, (n_img // groups) * H * W
            z, par, sync = conv_bn_stats(x0, weight, bias, geom, bn, groups, variant)
            if variant == "head":
                a = torch.empty((n_img, 1, H, W), dtype=F32, device=dev)
                _timed_hbm("bn_head_fwd", 2.0 * z.numel() + 4.0 * pixels,
                           lambda: L.check(K.uclstm_bn_head_fwd(_p(z), _p(par[0]), _p(par[1]), _p(head_w), _p(head_b), _p(a), pixels, ppg,
                                                                Cop, Co, _stream()), "bn_head_fwd"))
            elif variant == "pool":
                a = torch.empty_like(z)
                pooled = torch.empty((n_img, H // 2, W // 2, Cop), dtype=z.dtype, device=dev)
                _timed_hbm("bn_apply_relu_pool", 4.5 * z.numel(),
                           lambda: L.check(K.uclstm_bn_apply_relu_pool(_p(z), _p(a), _p(pooled), _p(par[0]), _p(par[1]), n_img, H, W, Cop,
                                                                       groups, _stream()), "bn_apply_relu_pool"))
            else:
                a = bn_relu(z, par, groups)
            ctx.save_for_backward(x0, x1, weight, z, par, gamma, beta, bias, head_w, head_b)
            if need_bw:
                note_use(weight, gamma, beta, bias, head_w, head_b)
        else:
            a = conv_bn_fold(x0, weight, bias, geom, bn, True)
            ctx.save_for_backward(x0, x1, weight, None, None, gamma, beta, bias, None, None)
        ctx.cfg = (tuple(c_valid), tuple(off), groups, training, im2col, Co, Ci_total, bias is not None)
        ctx.variant, ctx.sync_bn, ctx.pool_act = variant, sync, None
        if not pool:
            return a
        if variant != "pool":           # evaluation mode, odd sizes: the stand-alone pooling kernel on the finished activation
            pooled = _maxpool2_fwd(a)
            if need_bw:
                ctx.pool_act = a
        return a, pooled

    @staticmethod
    def _bn_backward(ctx, z, par, head_w, head_b, da, dp):
        """Part 1: (dz, sums, d_head_w, d_head_b) -- the gradient of the conv output and the per-group sums (dbeta, dgamma)."""
        groups, training, Co = ctx.cfg[2], ctx.cfg[3], ctx.cfg[5]
        variant = ctx.variant if (ctx.variant != "pool" or dp is not None) else "plain"          # pooled output unused
        if variant == "plain":
            if dp is not None:
                # pooling not fused (odd sizes / evaluation-mode statistics path): the stand-alone max-pool backward kernel first
                da = _maxpool2_bwd(ctx.pool_act, dp, da)
            return bn_relu_backward(z, par, da, groups, training, ctx.sync_bn) + (None, None)
        (n_img, H, W, Cop), dev = z.shape, z.device
        pixels, ppg = n_img * H * W, (n_img // groups) * H * W
        sums = torch.empty((groups, Cop, 2), dtype=F32, device=dev)
        partials = torch.empty((int(L.lib.uclstm_bn_bwd_reduce_rows(pixels, ppg)), Cop, 2), dtype=F32, device=dev)
        K = _k(z)
        dz = torch.empty_like(z)
        pz, pq = _p(z), (_p(par[0]), _p(par[1]), _p(par[2]), _p(par[3]))
        d_head_w = d_head_b = None
        if variant == "head":
            # fused output head: `da` is dy f32 [n_img, 1, H, W]; the activation gradient bf16(dy * w) is formed on the fly
            dy = _dev(da.contiguous().float(), F32, "dy")
            direct = direct_grad_pair(head_w, head_b, ctx.needs_input_grad[15], ctx.needs_input_grad[16])
            dwh = direct[0] if direct else torch.zeros_like(head_w, memory_format=torch.contiguous_format)
            dbh = direct[1] if (direct and head_b is not None) else torch.zeros((1,), dtype=F32, device=dev)
            if _DETERMINISTIC:
                # the head's Co + 1 columns go through partial rows of their own and are finished in row order (dwh / dbh keep +=)
                head_partials = torch.empty((partials.shape[0], Co + 1), dtype=F32, device=dev)
                _log_reduce("bn_head_bwd_reduce_ordered")
                _timed_hbm("bn_head_bwd_reduce", 2.0 * z.numel() + 4.0 * pixels,
                           lambda: L.check(L.lib.uclstm_bn_head_bwd_reduce_ordered(
                               pz, _p(dy), *pq, _p(head_w), _p(partials), _p(head_partials),
                               _p(sums), _p(dwh), _p(dbh), pixels, ppg, Cop, Co, L.act_type(z.dtype), _stream()), "bn_head_bwd_reduce_ordered"))
            else:
                _log_reduce("bn_head_bwd_reduce")
                _timed_hbm("bn_head_bwd_reduce", 2.0 * z.numel() + 4.0 * pixels,
                           lambda: L.check(K.uclstm_bn_head_bwd_reduce(pz, _p(dy), *pq, _p(head_w), _p(partials), _p(sums), _p(dwh), _p(dbh),
                                                                       pixels, ppg, Cop, Co, _stream()), "bn_head_bwd_reduce"))
            if direct:
                grad_written(head_w)
                if head_b is not None:
                    grad_written(head_b)
            else:
                d_head_w = dwh if ctx.needs_input_grad[15] else None
                d_head_b = dbh if (head_b is not None and ctx.needs_input_grad[16]) else None
            kind, nbytes = "bn_head_bwd_apply", 4.0 * z.numel() + 4.0 * pixels
            apply = lambda s: K.uclstm_bn_head_bwd_apply(pz, _p(dy), *pq, _p(s), _p(head_w), _p(dz), pixels, ppg, Cop, Co, _stream())
        else:
            # pooling fused: the gradient of the activation is (skip gradient) + scatter(dp), formed inside the BatchNorm kernels
            dsk = None if da is None else da.contiguous()
            dp = dp.contiguous()
            prt = torch.empty((int(L.lib.uclstm_bn_pool_bwd_rows(n_img, H, W, Cop, groups)), Cop, 2), dtype=F32, device=dev)
            _timed_hbm("bn_pool_bwd_reduce", (4.5 if dsk is not None else 2.5) * z.numel(),
                       lambda: L.check(K.uclstm_bn_pool_bwd_reduce(pz, _p(dsk), _p(dp), *pq, _p(prt), _p(sums), n_img, H, W, Cop, groups,
                                                                   _stream()), "bn_pool_bwd_reduce"))
            kind, nbytes = "bn_pool_bwd_apply", (6.5 if dsk is not None else 4.5) * z.numel()
            apply = lambda s: K.uclstm_bn_pool_bwd_apply(pz, _p(dsk), _p(dp), *pq, _p(s), _p(dz), n_img, H, W, Cop, groups, _stream())
        # the sums the apply pass takes: as in bn_relu_backward
        if ctx.sync_bn is not None:
            sums_dz = _bn_bwd_sums_over_ranks(sums, ctx.sync_bn, variant)
        else:
            sums_dz = sums if training else torch.zeros_like(sums)
        _timed_hbm(kind, nbytes, lambda: L.check(apply(sums_dz), kind))
        return dz, sums, d_head_w, d_head_b

    @staticmethod
    def _param_grads(ctx, dz, sums, gamma, beta, bias):
        """Part 2: (dbias, dgamma, dbeta) for autograd; None for a frozen parameter (requires_grad False: fine-tuning -- nothing
        is launched for it; bias, gamma and beta are independent of each other) and for one whose attached gradient was written."""
        (_, _, _, training, _, Co, _, has_bias), dev = ctx.cfg, dz.device
        need_b, need_gamma, need_beta = ctx.needs_input_grad[3:6]
        dgamma, dbeta, direct = bn_param_grads(need_gamma, need_beta, gamma, beta, sums, Co)
        dbias = None
        if need_b and has_bias:
            # training: the conv bias feeds BatchNorm, which removes any per-channel constant -- its gradient is analytically 0.
            # With frozen statistics it is the column sum of dz.
            g_bias = direct_grad(bias) if direct else None
            if not training:
                dbias = colsum(dz)[:Co].contiguous()
            elif g_bias is None:
                dbias = torch.zeros((Co,), dtype=F32, device=dev)
            if g_bias is not None:
                if dbias is not None:
                    g_bias.add_(dbias)
                grad_written(bias)                          # training: += 0
                dbias = None
        return dbias, dgamma, dbeta

    @staticmethod
    def backward(ctx, da, dp=None):
        x0, x1, weight, z, par, gamma, beta, bias, head_w, head_b = ctx.saved_tensors
        c_valid, off, _, _, im2col, _, _, _ = ctx.cfg
        dz, sums, d_head_w, d_head_b = ConvBNReLU._bn_backward(ctx, z, par, head_w, head_b, da, dp)
        dbias, dgamma, dbeta = ConvBNReLU._param_grads(ctx, dz, sums, gamma, beta, bias)
        # part 3: the weight gradient (not for a frozen weight) and the input gradients
        dweight = dx0 = dx1 = None
        if ctx.needs_input_grad[2]:
            dweight = conv_wgrad(weight, conv_geometry(x0, x1, weight, c_valid, off, im2col_pack_desc if im2col else None), dz)
        if ctx.needs_input_grad[0] and not im2col:
            dx0 = conv3x3_dgrad(dz, weight, x0, c_valid[0])
        if x1 is not None and ctx.needs_input_grad[1]:
            dx1 = conv3x3_dgrad(dz, weight, x1, c_valid[1], c_valid[0] * 9, -off[0], -off[1])
        return dx0, dx1, dweight, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None, None, d_head_w, d_head_b, None


# ---------------------------------------------------------------------------------------------
# MaxPool2d(2)  (train/unet.py:81)
# ---------------------------------------------------------------------------------------------
def _maxpool2_fwd(a: torch.Tensor) -> torch.Tensor:
    _dev(a, ACT, "activation")
    N, H, W, Cp = a.shape
    p = torch.empty((N, H // 2, W // 2, Cp), dtype=a.dtype, device=a.device)
    L.check(_k(a).uclstm_maxpool2_fwd(_p(a), _p(p), N, H, W, Cp, _stream()), "maxpool2_fwd")
    return p


def _maxpool2_bwd(a: torch.Tensor, dp: torch.Tensor, dskip: Optional[torch.Tensor]) -> torch.Tensor:
    """Gradient of ``a`` from the gradient ``dp`` of MaxPool2d(2)(a) and ``dskip`` (or None), the gradient of its other use.
    Even sizes: the kernel writes every element and adds ``dskip`` itself.  Odd sizes: the last row / column lies in no window,
    so the result is zero-filled first and ``dskip`` added afterwards."""
    N, H, W, Cp = a.shape
    odd = bool(H % 2 or W % 2)
    da = torch.zeros_like(a) if odd else torch.empty_like(a)
    add = dskip.contiguous() if (dskip is not None and not odd) else None
    L.check(_k(a).uclstm_maxpool2_bwd(_p(a), _p(dp.contiguous()), _p(add), _p(da), N, H, W, Cp, _stream()), "maxpool2_bwd")
    return da if (dskip is None or add is not None) else da + dskip


class MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        ctx.save_for_backward(a)
        return _maxpool2_fwd(a)

    @staticmethod
    def backward(ctx, dp):
        return _maxpool2_bwd(ctx.saved_tensors[0], dp, None)


class MaxPool2Skip(torch.autograd.Function):
    """MaxPool2d(2) of ``a`` plus ``a`` itself as a second output (the skip connection): in the UNet every encoder output is
    used twice (train/unet.py:166-169), so its gradient is a sum of two tensors -- added inside the max-pool backward kernel
    instead of by autograd's separate elementwise add (one read + one write of the full-resolution tensor less)."""

    @staticmethod
    def forward(ctx, a):
        ctx.save_for_backward(a)
        return _maxpool2_fwd(a), a.view_as(a)

    @staticmethod
    def backward(ctx, dp, dskip):
        return dskip if dp is None else _maxpool2_bwd(ctx.saved_tensors[0], dp, dskip)


# ---------------------------------------------------------------------------------------------
# ConvTranspose2d(k=2, s=2)  (train/unet.py:90, :94)
# ---------------------------------------------------------------------------------------------
class ConvT2x2(_GradAwareFunction):
    @staticmethod
    def forward(ctx, x, weight, bias):
        _dev(x, ACT, "activation")
        Ci, Co = weight.shape[0], weight.shape[1]
        Cop = cpad(Co)
        N, h, w, _ = x.shape
        pd = convt_pack_desc(Ci, Co)
        wp = pack_weights(pd, weight, 0, x.dtype)
        bp = pack_bias(pd, bias) if bias is not None else None
        u = torch.empty((N, 2 * h, 2 * w, Cop), dtype=x.dtype, device=x.device)
        segs = [(u, t * Cop, (t + 1) * Cop, 0, 2, t // 2, t % 2) for t in range(4)]
        igemm_store([SrcView(x)], wp, (h, w), N, segs, ktap=1, pad=0, bias=bp)
        ctx.save_for_backward(x, weight, bias)
        ctx.has_bias = bias is not None
        if _will_backward(ctx):
            note_use(weight, bias)
        return u

    @staticmethod
    def backward(ctx, du):
        x, weight, bias = ctx.saved_tensors
        du = du.contiguous()
        Ci, Co = weight.shape[0], weight.shape[1]
        Cop = cpad(Co)
        N, h, w, _ = x.shape
        pd = convt_pack_desc(Ci, Co)
        segs = [(du, t * Cop, (t + 1) * Cop, 0, 2, t // 2, t % 2) for t in range(4)]
        dweight = dbias = None
        if ctx.needs_input_grad[1]:          # not for a frozen weight
            dweight = wgrad_into_param(weight, pd, [x, du], lambda: igemm_wgrad([SrcView(x)], segs, pd.N, pd.Ktot, (h, w), N, ktap=1, pad=0))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            dbias = bias_grad_from_colsum(du, bias, Co)
        dx = None
        if ctx.needs_input_grad[0]:
            dd = convt_dgrad_pack_desc(Ci, Co)
            wd = pack_weights(dd, weight, 0, du.dtype)
            dx = torch.empty_like(x)
            igemm_store([SrcView(du)], wd, (h, w), N, [(dx, 0, dd.N, 0, 1, 0, 0)], ktap=2, scale=2, pad=0)
        return dx, dweight, dbias


# ---------------------------------------------------------------------------------------------
# OutConv 1x1  (train/unet.py:101-107)
# ---------------------------------------------------------------------------------------------
class OutConv1x1(_GradAwareFunction):
    """16-bit NHWC in, f32 NCHW out (the model's public output dtype/layout)."""

    @staticmethod
    def forward(ctx, a, weight, bias):
        _dev(a, ACT, "activation")
        N, H, W, Cp = a.shape
        Co, Ci = weight.shape[0], weight.shape[1]
        y = torch.empty((N, Co, H, W), dtype=F32, device=a.device)
        L.check(_k(a).uclstm_outconv_fwd(_p(a), _p(weight), _p(bias), _p(y), N, H * W, Cp, Ci, Co, _stream()), "outconv_fwd")
        ctx.save_for_backward(a, weight, bias)
        ctx.has_bias = bias is not None
        if _will_backward(ctx):
            note_use(weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, weight, _ = ctx.saved_tensors
        N, H, W, Cp = a.shape
        # (the kernels take the parameter [Co, Ci, 1, 1] and its gradient as [Co, Ci])
        return head_backward(ctx, dy, "outconv_bwd", _k(a).uclstm_outconv_bwd, L.lib.uclstm_outconv_bwd_ordered,
                             (N, H * W, Cp, weight.shape[1], weight.shape[0]), lambda: L.lib.uclstm_outconv_bwd_ordered_rows(N, H * W),
                             spare=True)


def head_backward(ctx, dy, kind: str, atomic, ordered, geom: tuple, rows, *, spare: bool = False, timed: bool = False):
    """Backward of an f32 output head that saved ``(a, weight, bias)`` and set ``ctx.has_bias`` (OutConv1x1, resnet.Head3x3):
    ``(da, dweight, dbias)``.  ``atomic(a, weight, dy, da, dw, db, *geom, stream)`` ADDS its block sums into dw / db with float
    atomics and skips them when given no buffers (weight and bias frozen); deterministic mode takes
    ``ordered(a, weight, dy, da, partials, dw, db, accumulate, *geom, act type, stream)`` with ``rows()`` partial rows of
    (weight elements + Co) columns.  With attached f32 gradients (direct_grad_pair) the kernels add straight into them: no
    zero-fill, no accumulate kernels.  ``kind`` goes to _log_reduce (plus "_ordered").  ``spare``: the kernels get a scratch buffer
    for the weight gradient always and (atomic form) for the bias gradient always, where otherwise a gradient nobody wants gets
    none.  ``timed``: the launch is recorded in PROFILE_HBM as ``kind``."""
    a, weight, bias = ctx.saved_tensors
    dy = dy.contiguous().float()
    Co, dev, det = weight.shape[0], a.device, _DETERMINISTIC
    da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
    need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
    if not (need_w or need_b):
        if da is not None:
            L.check(atomic(_p(a), _p(weight), _p(dy), _p(da), None, None, *geom, _stream()), kind)
        return da, None, None
    direct = direct_grad_pair(weight, bias, need_w, need_b)
    gw, gb = direct or (None, None)
    fresh = torch.empty if det else torch.zeros          # the ordered form writes, the atomic form adds
    dw = gw if direct else (fresh(weight.shape, dtype=F32, device=dev) if (need_w or spare) else None)
    db = gb if (direct and ctx.has_bias) else (fresh((Co,), dtype=F32, device=dev) if (need_b or (spare and not det)) else None)
    if det:
        partials = torch.empty((int(rows()) * (weight.numel() + Co),), dtype=F32, device=dev)
        launch = lambda: L.check(ordered(_p(a), _p(weight), _p(dy), _p(da), _p(partials), _p(dw), _p(db), 1 if direct else 0, *geom,
                                         L.act_type(a.dtype), _stream()), kind + "_ordered")
    else:
        launch = lambda: L.check(atomic(_p(a), _p(weight), _p(dy), _p(da), _p(dw), _p(db), *geom, _stream()), kind)
    _log_reduce(kind + "_ordered" if det else kind)
    if timed:
        _timed_hbm(kind, 2.0 * a.numel() * (2 if da is not None else 1) + 4.0 * dy.numel(), launch)
    else:
        launch()
    if direct:
        grad_written(weight)
        if ctx.has_bias:
            grad_written(bias)
        return da, None, None
    return da, (dw if need_w else None), (db if need_b else None)


# ---------------------------------------------------------------------------------------------
# SpatialAttention  (train/unet.py:113-125)
# ---------------------------------------------------------------------------------------------
class SpatialAttn(_GradAwareFunction):
    """x * sigmoid(conv_kxk([mean_c x, max_c x])) on NHWC 16-bit activations; ``weight`` is the reference's [1,2,k,k] f32."""

    @staticmethod
    def forward(ctx, x, weight, channels):
        _dev(x, ACT, "activation")
        _dev(weight, F32, "attention weight")
        N, H, W, Cp = x.shape
        k = weight.shape[-1]
        dev = x.device
        out = torch.empty_like(x)
        att = torch.empty((N, H, W), dtype=F32, device=dev)
        desc = torch.empty((N, H, W, 2), dtype=F32, device=dev)
        arg = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        L.check(_k(x).uclstm_attention_fwd(_p(x), _p(weight), _p(out), _p(att), _p(desc), _p(arg), N, H, W, Cp, channels, k, _stream()),
                "attention_fwd")
        ctx.save_for_backward(x, weight, att, desc, arg)
        ctx.channels = channels
        if _will_backward(ctx):
            note_use(weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, att, desc, arg = ctx.saved_tensors
        dout = dout.contiguous()
        N, H, W, Cp = x.shape
        k = weight.shape[-1]
        dx = torch.empty_like(x)
        scratch = torch.empty((3 * N * H * W + 2,), dtype=F32, device=x.device)
        need_w = ctx.needs_input_grad[1]
        g = direct_grad(weight) if need_w else None
        dw = g if g is not None else (torch.empty_like(weight) if need_w else None)          # None (frozen weight): no dw kernel
        L.check(_k(x).uclstm_attention_bwd(_p(x), _p(dout), _p(weight), _p(att), _p(desc), _p(arg), _p(dx), _p(dw), int(g is not None),
                                           _p(scratch), N, H, W, Cp, ctx.channels, k, _stream()), "attention_bwd")
        if g is not None:
            grad_written(weight)
            return dx, None, None
        return dx, dw, None


# ---------------------------------------------------------------------------------------------
# ConvLSTM layer over a whole sequence  (train/unet.py:21-36 x T, :55-57)
# ---------------------------------------------------------------------------------------------
class _LstmLayerFwd:
    """The forward recurrence of ONE ConvLSTM layer: panels, state storage and the descriptors of every step.  ConvLSTMSeq.forward
    launches its steps one by one, convlstm_group_forward / convlstm_group_step those of 2 to 4 layers as group launches.

    x_all [T,B,H,W,Cxp]; h0 [B,H,W,Hdp] / c0 f32 or None (zero state).  State storage:
      training / plain    h_hist, c_hist of T+1 slots, slot 0 a copy of h0 / c0 (zeros for h0 = None; c_hist[0] is not read for c0 = None)
      direct (inference)  the same, but step 0 reads h0 / c0 where they lie (``in_place``; slot 0 is then not written)
      out = (h, c)        one step with a carried state that writes the caller's buffers (h_out must not be h0: the convolution reads
                          h0's neighbourhoods while h_out is written; c_out may be c0 itself, the cell update is element-wise)
    ``hoist`` (single sequences only, T >= 2): W_x * x_t for ALL timesteps as one GEMM over T*B*H*W pixels, launched here (f32
    pre-activations in panel-row order); the recurrence then multiplies only by W_h: K and the weight bytes re-read per step halve
    (SURVEY.md section 7-4)."""

    def __init__(self, x_all, h0, c0, weight, bias, Hd, Cx, need_grad, out=None, hoist=False, in_place=True):
        _dev(x_all, ACT, "x_all")
        adt, dev = x_all.dtype, x_all.device
        T, B, H, W, Cxp = x_all.shape
        self.x_all, self.h0, self.T, self.B, self.H, self.W = x_all, h0, T, B, H, W
        self.ks = ks = weight.shape[-1]
        self.Hdp = Hdp = cpad(Hd)
        self.pixels = pixels = B * H * W
        pd = lstm_pack_desc(Hd, Cx, ks)
        self.bp = pack_bias(pd, bias) if bias is not None else None
        state = (B, H, W, Hdp)
        fits = lambda t, dt: t.is_contiguous() and t.dtype == dt and tuple(t.shape) == state
        if out is not None:
            if need_grad or T != 1 or h0 is None:
                raise L.UclstmError("ConvLSTMSeq: out= is for one-step inference with a carried state")
            if not (fits(out[0], adt) and fits(out[1], F32)):
                raise L.UclstmError("ConvLSTMSeq: out buffers must be contiguous [B,H,W,Hd_p] (h: activation dtype, c: f32)")
            if out[0].data_ptr() == h0.data_ptr():
                raise L.UclstmError("ConvLSTMSeq: h_out aliases h0")
        # inference (nothing saved): step 0 reads the caller's state tensors where they lie instead of copies in slot 0
        direct = in_place and not need_grad and h0 is not None and fits(h0, adt) and (c0 is None or fits(c0, F32))
        if out is not None and not direct:
            raise L.UclstmError("ConvLSTMSeq: out= needs the carried state as contiguous [B,H,W,Hd_p] tensors (h: activation dtype, c: f32)")
        self.h_hist = torch.empty((T + 1,) + state, dtype=adt, device=dev) if out is None else (None, out[0])
        self.c_hist = torch.empty((T + 1,) + state, dtype=F32, device=dev) if out is None else (None, out[1])
        if h0 is None:
            self.h_hist[0].zero_()
        elif not direct:
            self.h_hist[0].copy_(h0)
        if c0 is not None and not direct:
            self.c_hist[0].copy_(c0)
        self.h_first = h0 if direct else self.h_hist[0]
        self.c_first = None if c0 is None else (c0 if direct else self.c_hist[0])
        self.gates = torch.empty((T, B, H, W, 4, Hdp), dtype=adt, device=dev) if need_grad else None
        self.pre_x = None
        if hoist and T >= 2:
            wx = pack_weights(lstm_half_pack_desc(Hd, Cx, "x", ks), weight, 0, adt)
            self.wp = pack_weights(lstm_half_pack_desc(Hd, Cx, "h", ks), weight, 0, adt)
            N = self.wp.shape[0]
            pre_x = torch.empty((1, T * pixels, N), dtype=F32, device=dev)
            for i0, i1 in _img_chunks(T * B, 1, max(_bytes_per_img(x_all[0]), H * W * N * 4), "convlstm x half"):
                igemm_atomic([SrcView(x_all.view(T * B, H, W, Cxp)[i0:i1])], wx, (H, W), i1 - i0,
                             pre_x[:, i0 * H * W:i1 * H * W], 1, ktap=ks, pad=ks // 2, slabs=True, kind="igemm_fwd_xhoist")
            self.pre_x = pre_x.view(T, pixels, N)
        else:
            self.wp = pack_weights(pd, weight, 0, adt)
        self.N, self.Ktot = self.wp.shape
        # this layer's entry of plan_group_ksplit's argument: (128 x 256 output tiles, chunks of 64 channels x 9 taps)
        self.group_plan_input = ((self.N + 127) // 128) * (pixels // 256), self.Ktot // (64 * 9)
        # the point-wise kernel's arguments: the constants here, the step's slots in step()
        self.pw = a = L.LstmFwdPwArgs()
        a.clear, a.pixels, a.Hd_p = 0, pixels, Hdp
        a.bias = None if self.bp is None else self.bp.data_ptr()

    def split(self, ksplit: int) -> None:
        """K ranges per step, from the caller's planner.  More than one: one f32 slab per K range (plain stores; the point-wise
        kernel adds them): no atomics, nothing to zero."""
        self.ksplit = ksplit
        nsl = ksplit_used(self.Ktot, ksplit, self.ks) if ksplit > 1 else 0
        self.pre = torch.empty((nsl, self.pixels, self.N), dtype=F32, device=self.x_all.device) if ksplit > 1 else None

    def step(self, t: int):
        """Step t as (igemm item, point-wise arguments): the fused cell (item, None), split-K slabs + the point-wise kernel
        (item, args), or -- hoisted with a zero initial state (train/unet.py:23-25): W_h * 0 = 0, the step is the point-wise update
        of W_x * x_0 -- (None, args).  The arguments are this layer's one struct: use them before the next call."""
        h_prev, c_prev = (self.h_first, self.c_first) if t == 0 else (self.h_hist[t], self.c_hist[t])
        c_out, h_out = self.c_hist[t + 1], self.h_hist[t + 1]
        g_t = None if self.gates is None else self.gates[t]
        hoist = self.pre_x is not None
        px_t = self.pre_x[t] if hoist else None
        ks = self.ks
        alone = hoist and t == 0 and self.h0 is None
        if self.ksplit == 1 and not alone:
            return _lstm_desc(None if hoist else self.x_all[t], h_prev, self.wp, self.bp, c_prev, c_out, h_out, g_t, ks, pre_add=px_t), None
        pre = None if alone else self.pre
        item = None if alone else _atomic_desc(([] if hoist else [SrcView(self.x_all[t])]) + [SrcView(h_prev)], self.wp, (self.H, self.W),
                                               self.B, pre, self.ksplit, ktap=ks, pad=ks // 2, slabs=True)
        a = self.pw
        a.pre, a.nslab, a.slab = (None, 0, 0) if alone else (pre.data_ptr(), pre.shape[0], pre.stride(0))
        a.pre_add = None if px_t is None else px_t.data_ptr()
        a.c_prev = None if c_prev is None else c_prev.data_ptr()
        a.c_out, a.h_out = c_out.data_ptr(), h_out.data_ptr()
        a.gates_out = None if g_t is None else g_t.data_ptr()
        return item, a


def _lstm_launch_one(K, item, pw) -> None:
    """One step of one layer: a launch of its own, then the point-wise kernel where the step has one."""
    if item is not None:
        _igemm_launch(item, K, *(("igemm_fwd_lstm", "igemm_fwd(lstm)") if pw is None else ("igemm_fwd_atomic", "igemm_fwd(atomic)")))
    if pw is not None:
        L.check(K.uclstm_lstm_fwd_pointwise(pw.pre, pw.nslab, pw.slab, pw.clear, pw.pre_add, pw.bias, pw.c_prev, pw.c_out, pw.h_out,
                                            pw.gates_out, pw.pixels, pw.Hd_p, _stream()), "lstm_fwd_pointwise")


def _lstm_launch_group(K, steps) -> None:
    """One step of several layers (``steps``: what each layer's step() returned): ONE group launch, then at most one point-wise launch."""
    igemm_group([item for item, _ in steps], K)
    pws = [pw for _, pw in steps if pw is not None]
    if pws:
        L.check(K.uclstm_lstm_fwd_pointwise_group((L.LstmFwdPwArgs * len(pws))(*pws), len(pws), _stream()), "lstm_fwd_pointwise_group")


class ConvLSTMSeq(torch.autograd.Function):
    """All T steps of one ConvLSTM layer.

    x_all bf16 [T,B,H,W,Cxp]; h0 bf16 [B,H,W,Hdp] / c0 f32 or None (zero state).
    Returns (h_all bf16 [T,B,H,W,Hdp], c_T f32 [B,H,W,Hdp]); h_T is h_all[T-1].
    Forward: one fused kernel per step (gate conv over (x_t, h_{t-1}) + nonlinearities + cell
    update), post-activation gates kept in bf16 for the backward pass when training.
    Backward: per step (reverse) a point-wise kernel + the h-part input-gradient GEMM; the x-part
    input gradient and the weight gradient are batched over all T after the loop.
    """

    @staticmethod
    def forward(ctx, x_all, h0, c0, weight, bias, Hd, Cx, need_grad, out=None):
        ctx.set_materialize_grads(False)
        m = _LstmLayerFwd(x_all, h0, c0, weight, bias, Hd, Cx, need_grad, out, hoist=HOIST_X)
        # Per-step GEMM M = B*H*W.  When its tile grid cannot fill the chip (bottleneck LSTM: M = 512), run the gate
        # convolution as split-K partial tiles in f32 slabs and apply the cell update in a point-wise kernel; otherwise one
        # fused kernel per step (gates never leave registers).
        m.split(split_k_factor(m.pixels, m.N, m.Ktot // 64))
        K = _k(x_all)
        for t in range(m.T):
            _lstm_launch_one(K, *m.step(t))
        if RECURRENCE_TRACE is not None:
            RECURRENCE_TRACE.append(("fwd", m.h_hist, m.c_hist, m.gates))
        if need_grad:
            ctx.save_for_backward(x_all, weight, m.h_hist, m.c_hist, m.gates, bias)
            ctx.cfg = (Hd, Cx, c0 is not None, bias is not None, m.ks)
            note_use(weight, bias)
        if out is not None:
            return out[0].unsqueeze(0), out[1]
        return m.h_hist[1:], m.c_hist[m.T]

    @staticmethod
    def backward(ctx, dh_all, dc_T):
        x_all, weight, h_hist, c_hist, gates, bias = ctx.saved_tensors
        Hd, Cx, has_c0, has_bias, ks = ctx.cfg
        T, B, H, W, Cxp = x_all.shape
        Hdp = cpad(Hd)
        dev = x_all.device
        pixels = B * H * W
        dh_all = None if dh_all is None else dh_all.contiguous()
        adt = x_all.dtype
        K = _k(x_all)
        dgates = torch.empty((T, B, H, W, 4 * Hdp), dtype=adt, device=dev)
        dc = torch.empty((B, H, W, Hdp), dtype=F32, device=dev)
        dc_zero = dc_T is None
        if not dc_zero:
            dc.copy_(dc_T)
        ddh = lstm_dgrad_pack_desc(Hd, Cx, Hd, ks)
        wd_h = pack_weights(ddh, weight, Cx * ks * ks, adt)
        dh_rec = None
        # recurrent gradient dh_{t-1} = W_h^T (*) dgates_t: M = B*H*W pixels, N = Hd, K = 9*4*Hd.  Small M -> split-K with
        # f32 atomics into dh (read back as f32 by the next step's point-wise kernel); else a plain bf16 store.
        ksplit = split_k_factor(pixels, ddh.N, ddh.Ktot // 64)
        # split-K: one f32 slab per K range, plain stores; the point-wise kernel of the next (earlier) timestep adds them.
        # Two buffers alternate so that step t's GEMM never writes what step t+1's point-wise kernel still reads.
        nsl = ksplit_used(ddh.Ktot, ksplit, ks) if ksplit > 1 else 1
        if ksplit > 1:
            buf = [torch.empty((nsl, B, H, W, Hdp), dtype=F32, device=dev) for _ in range(2)]
        else:
            buf = [torch.empty((B, H, W, Hdp), dtype=adt, device=dev) for _ in range(2)]
        need_h0 = ctx.needs_input_grad[1]
        for t in range(T - 1, -1, -1):
            c_prev = c_hist[t] if (has_c0 or t > 0) else None
            L.check(K.uclstm_lstm_bwd_pointwise(_p(gates[t]), _p(c_prev), _p(c_hist[t + 1]),
                                                    _p(dh_all[t]) if dh_all is not None else None, _p(dh_rec),
                                                    1 if ksplit > 1 else 0, nsl, pixels * Hdp, _p(dc),
                                                    int(dc_zero), _p(dgates[t]), pixels, Hdp, _stream()), "lstm_bwd_pointwise")
            dc_zero = False
            if t > 0 or need_h0:
                dh_rec = buf[t & 1]
                if ksplit > 1:
                    igemm_atomic([SrcView(dgates[t])], wd_h, (H, W), B, dh_rec.view(nsl, pixels, Hdp), ksplit, ktap=ks, pad=ks // 2,
                                 slabs=True)
                else:
                    igemm_store([SrcView(dgates[t])], wd_h, (H, W), B, [(dh_rec, 0, ddh.N, 0, 1, 0, 0)], ktap=ks, pad=ks // 2)
        if RECURRENCE_TRACE is not None:
            RECURRENCE_TRACE.append(("bwd", dgates))
        dg_flat = dgates.view(T * B, H, W, 4 * Hdp)
        x_flat = x_all.reshape(T * B, H, W, Cxp)
        hprev_flat = h_hist[:T].reshape(T * B, H, W, Hdp)
        dweight = None
        if ctx.needs_input_grad[3]:          # a frozen gate weight launches neither the weight-gradient GEMM nor its un-pack
            ud = lstm_wgrad_unpack_desc(Hd, Cx, ks)
            dweight = wgrad_into_param(weight, ud, [x_all, h_hist, dgates],
                                       lambda: igemm_wgrad([SrcView(x_flat), SrcView(hprev_flat)], [(dg_flat, 0, 4 * Hdp, 0, 1, 0, 0)],
                                                           ud.N, ud.Ktot, (H, W), T * B, ktap=ks, pad=ks // 2))
        dbias = None
        if has_bias and ctx.needs_input_grad[4]:
            if Hdp == Hd:           # dgates columns are (gate, hidden channel) = the bias order of train/unet.py:29
                dbias = bias_grad_from_colsum(dg_flat, bias, 4 * Hd)
            else:
                dbias = colsum(dg_flat).view(4, Hdp)[:, :Hd].reshape(4 * Hd).contiguous()
        dx_all = None
        if ctx.needs_input_grad[0]:
            ddx = lstm_dgrad_pack_desc(Hd, Cx, Cx, ks)
            wd_x = pack_weights(ddx, weight, 0, adt)
            dx_all = torch.empty_like(x_all)
            igemm_store([SrcView(dg_flat)], wd_x, (H, W), T * B, [(dx_all.view(T * B, H, W, Cxp), 0, ddx.N, 0, 1, 0, 0)], ktap=ks,
                        pad=ks // 2)
        dh0 = (dh_rec if dh_rec.dtype == adt else dh_rec.sum(dim=0).to(adt)) if need_h0 else None
        dc0 = dc if (has_c0 and ctx.needs_input_grad[2]) else None
        return dx_all, dh0, dc0, dweight, dbias, None, None, None


# ---------------------------------------------------------------------------------------------
# Several independent ConvLSTMs advancing in lockstep (train/unet.py:185-191 runs temporal, lstm_skip3, lstm_skip2 one after
# the other; they do not depend on each other)
# ---------------------------------------------------------------------------------------------
GROUP_LSTM = os.environ.get("UCLSTM_GROUP_LSTM", "1") != "0"
FUSE_POOL = os.environ.get("UCLSTM_FUSE_POOL", "1") != "0"          # MaxPool2d(2) fused into the BatchNorm stage that feeds it (training)
FUSE_HEAD = os.environ.get("UCLSTM_FUSE_HEAD", "1") != "0"          # 1x1 output convolution fused into the last BatchNorm stage (training)
_GROUP_PLANS: dict = {}
_CUS = 256
_BLOCK_OVERHEAD_STEPS = 12.0          # prologue + epilogue of a patch-shape block in units of one K-step (~10 us / 0.87 us)


def _lpt_makespan(blocks: List[Tuple[float, int]], cus: int = _CUS) -> float:
    """Makespan of (duration, count) block classes handed out longest first to ``cus`` one-block-at-a-time workers."""
    free = [0.0] * cus
    for dur, cnt in sorted(blocks, reverse=True):
        for _ in range(cnt):
            t = heapq.heappop(free)
            heapq.heappush(free, t + dur)
    return max(free)


def plan_group_ksplit(members: Sequence[Tuple[int, int]]) -> Tuple[int, ...]:
    """K ranges per member of a group launch.  ``members``: (tiles, chunks) = 128 x 256 output tiles and (source, 64-channel)
    K chunks of each member's GEMM; a block of member i runs ceil(chunks_i / ksplit_i) chunks of 9 K-steps plus a fixed
    prologue / epilogue.  Exhaustive search over ksplit <= 16 per member for the smallest longest-block-first makespan on the
    256 CUs (every extra K range also costs an f32 slab round trip, priced at a quarter of a K-step per slab and tile row)."""
    key = tuple(members)
    hit = _GROUP_PLANS.get(key)
    if hit is not None:
        return hit
    options = []
    for tiles, chunks in members:
        ks = sorted({k for k in range(1, min(chunks, 16) + 1) if (chunks + k - 1) // k != (chunks + k - 2) // max(k - 1, 1) or k == 1})
        options.append(ks)
    best, best_cost = None, None
    for combo in itertools.product(*options):
        blocks, slab_cost = [], 0.0
        for (tiles, chunks), k in zip(members, combo):
            cper = (chunks + k - 1) // k
            used = (chunks + cper - 1) // cper
            full, rem = divmod(chunks, cper)
            blocks.append((9.0 * cper + _BLOCK_OVERHEAD_STEPS, tiles * full))
            if rem:
                blocks.append((9.0 * rem + _BLOCK_OVERHEAD_STEPS, tiles))
            if used > 1:
                slab_cost += 0.25 * used * tiles / _CUS * 8
        cost = _lpt_makespan(blocks) + slab_cost
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = combo, cost
    _GROUP_PLANS[key] = best
    return best


def _group_shapes_ok(ms) -> bool:
    """Can 2 to 4 layers' step GEMMs take the patch shape together?  ``ms``: (x [..., B,H,W,Cxp], weight, Hd) per layer: one dtype, 3x3
    gate convolution, channel counts multiples of 64 (no padded hidden channels), B*H*W a multiple of 256."""
    if not GROUP_LSTM or not 2 <= len(ms) <= 4:
        return False
    for x, weight, Hd in ms:
        B, H, W, Cxp = x.shape[-4:]
        if x.dtype != ms[0][0].dtype or weight.shape[-1] != 3 or cpad(Hd) != Hd or Hd % 64 or Cxp % 64 or (B * H * W) % 256:
            return False
    return True


def _group_split(ms) -> None:
    """K ranges of every layer of a group from plan_group_ksplit."""
    for m, ksplit in zip(ms, plan_group_ksplit([m.group_plan_input for m in ms])):
        m.split(ksplit)


def convlstm_group_forward(members, need_grad: bool):
    """All T forward steps of n independent single-layer ConvLSTMs with ONE group launch per timestep (uclstm_igemm_fwd_group)
    instead of n launches.  ``members``: (x_all [T,B,H,W,Cxp], h0, c0, weight, bias, Hd, Cx) each; returns per member
    (h_hist [T+1,...], c_hist [T+1,...], gates or None) -- exactly what ConvLSTMSeq.forward keeps -- so that every member gets
    its OWN autograd node (ConvLSTMSeqPre) and its backward pass runs when ITS gradient arrives, as with separate sequences.
    (One node for the whole group was measured: backward 21.3 -> 21.8 ms, because the three weight-gradient GEMMs then reach
    the side stream together at the end instead of each overlapping the next LSTM's backward recurrence.)
    Same arithmetic as ConvLSTMSeq: a member's step is the fused cell kernel or split-K slabs + the point-wise kernel; only the
    K-range counts are planned for the group (plan_group_ksplit), i.e. results agree to f32 summation order of the K ranges."""
    ms = [_LstmLayerFwd(*mem, need_grad, in_place=False) for mem in members]       # the caller gets the histories: slot 0 is the state
    _group_split(ms)
    K = _k(ms[0].x_all)
    for t in range(ms[0].T):
        _lstm_launch_group(K, [m.step(t) for m in ms])
    if RECURRENCE_TRACE is not None:
        for m in ms:
            RECURRENCE_TRACE.append(("fwd", m.h_hist, m.c_hist, m.gates))
    return [(m.h_hist, m.c_hist, m.gates) for m in ms]


def convlstm_group_step(members) -> bool:
    """ONE inference step of n independent single-layer ConvLSTMs with carried state as one group launch (streaming rollout,
    BASELINE configs[4]).  ``members``: (x_t [B,H,W,Cxp], h_prev, c_prev, h_out, c_out, weight, bias, Hd, Cx); the new state is
    written into h_out / c_out (h_out must not alias h_prev; c_out may be c_prev).  Returns False -- nothing launched -- when the
    members cannot form a group (the caller then steps them one by one)."""
    if not _group_shapes_ok([(mem[0], mem[5], mem[7]) for mem in members]):
        return False
    if any(h_prev is None or c_prev is None or h_out.data_ptr() == h_prev.data_ptr() for _, h_prev, c_prev, h_out, *_ in members):
        return False
    ms = [_LstmLayerFwd(x_t.unsqueeze(0), h_prev, c_prev, weight, bias, Hd, Cx, False, (h_out, c_out))
          for x_t, h_prev, c_prev, h_out, c_out, weight, bias, Hd, Cx in members]
    _group_split(ms)
    steps = [m.step(0) for m in ms]
    if not group_launchable([item[0] for item, _ in steps]):
        return False
    _lstm_launch_group(_k(ms[0].x_all), steps)
    return True


_TICK_MAX = 4          # members per group launch (GROUP_MAX of csrc/igemm_fwd.hip) and per point-wise group launch


def _tick_kind(desc) -> str:
    """Which launch of convlstm_tick a step descriptor takes -- the library's own answer: "patch" (uclstm_igemm_fwd_group takes
    it), "tap" (uclstm_igemm_fwd_group_tap does) or "single" (neither: a launch of its own)."""
    one = (L.IgemmDesc * 1)(desc)
    if int(L.lib.uclstm_igemm_fwd_group_blocks(one, 1)) > 0:
        return "patch"
    if int(L.lib.uclstm_igemm_fwd_group_tap_blocks(one, 1)) > 0:
        return "tap"
    return "single"


def convlstm_tick(members) -> None:
    """ONE inference step of n independent single-layer ConvLSTMs with carried state, whatever their sizes: the five recurrences
    of resnet.PretrainedTemporalUNet, whose step GEMMs run on B*h*w = 1024 ... 4 pixels at 64 x 64.  ``members``: what
    convlstm_group_step takes, (x_t [B,H,W,Cxp], h_prev, c_prev, h_out, c_out, weight, bias, Hd, Cx); the new state is written
    into h_out / c_out (h_out must not alias h_prev; c_out may be c_prev).  Every member is launched:

      patch-shape steps     uclstm_igemm_fwd_group, up to four per launch; two or more in a launch take their K ranges from
                            plan_group_ksplit, as in convlstm_group_step
      128 x 128 3x3 steps   uclstm_igemm_fwd_group_tap, up to four per launch, each with the K split it has alone
                            (split_k_factor), so its result is bit-identical to stepping it alone
      anything else         (a 5x5 cell, a 64 x 256 split-K step) one by one

    and the split members of both group kinds share uclstm_lstm_fwd_pointwise_group launches of up to four.  ``GROUP_LSTM =
    False``: every member one by one (the A/B baseline).  LAUNCH_LOG gets ("tick", kind, members) per launch, kind = "patch" /
    "tap" / "single" / "pointwise"."""
    if not members:
        return
    for x_t, h_prev, c_prev, h_out, c_out, *_ in members:
        if h_prev is None or c_prev is None or h_out is None or c_out is None:
            raise L.UclstmError("convlstm_tick: every member carries its state (h_prev, c_prev) and names its output buffers")
        if h_out.data_ptr() == h_prev.data_ptr():
            raise L.UclstmError("convlstm_tick: h_out aliases h_prev")
    _same_act_dtype([mem[0] for mem in members], "convlstm_tick")
    ms = [_LstmLayerFwd(x_t.unsqueeze(0), h_prev, c_prev, weight, bias, Hd, Cx, False, (h_out, c_out))
          for x_t, h_prev, c_prev, h_out, c_out, weight, bias, Hd, Cx in members]
    K = _k(ms[0].x_all)
    buckets = {"patch": [], "tap": [], "single": []}
    for m in ms:
        m.split(split_k_factor(m.pixels, m.N, m.Ktot // 64))
        step = m.step(0)
        buckets[_tick_kind(step[0][0]) if GROUP_LSTM else "single"].append((m, step))

    def log(kind: str, n: int) -> None:
        if LAUNCH_LOG is not None:
            LAUNCH_LOG.append(("tick", kind, n))

    pws = []
    for kind in ("patch", "tap"):
        for i in range(0, len(buckets[kind]), _TICK_MAX):
            chunk = buckets[kind][i:i + _TICK_MAX]
            if kind == "patch" and len(chunk) > 1:          # K ranges planned for the launch; the point-wise struct is per layer
                _group_split([m for m, _ in chunk])
                chunk = [(m, m.step(0)) for m, _ in chunk]
            igemm_group([step[0] for _, step in chunk], K, tap=kind == "tap")
            log(kind, len(chunk))
            pws += [step[1] for _, step in chunk if step[1] is not None]
    for i in range(0, len(pws), _TICK_MAX):
        chunk = pws[i:i + _TICK_MAX]
        L.check(K.uclstm_lstm_fwd_pointwise_group((L.LstmFwdPwArgs * len(chunk))(*chunk), len(chunk), _stream()), "lstm_fwd_pointwise_group")
        log("pointwise", len(chunk))
    for _, step in buckets["single"]:
        _lstm_launch_one(K, *step)
        log("single", 1)


class ConvLSTMSeqPre(torch.autograd.Function):
    """ConvLSTMSeq whose forward pass has already been computed (convlstm_group_forward): the node only records what
    ConvLSTMSeq.forward would have saved; its backward IS ConvLSTMSeq.backward."""

    @staticmethod
    def forward(ctx, x_all, h0, c0, weight, bias, Hd, Cx, need_grad, h_hist, c_hist, gates):
        ctx.set_materialize_grads(False)
        T = x_all.shape[0]
        if need_grad:
            ctx.save_for_backward(x_all, weight, h_hist, c_hist, gates, bias)
            ctx.cfg = (Hd, Cx, c0 is not None, bias is not None, weight.shape[-1])
            note_use(weight, bias)
        return h_hist[1:], c_hist[T]

    @staticmethod
    def backward(ctx, dh_all, dc_T):
        return ConvLSTMSeq.backward(ctx, dh_all, dc_T) + (None, None, None)


def convlstm_group_ok(members) -> bool:
    """Can these (x_all, h0, c0, weight, bias, Hd, Cx) single-layer ConvLSTMs run through convlstm_group_forward?  Every per-step
    GEMM must take the patch shape (_group_shapes_ok) -- checked with the library's own planner on the step-0 descriptors -- and all
    members share T, B and the activation dtype."""
    try:
        x0 = members[0][0]
        if any(m[0].dim() != 5 or m[0].shape[:2] != x0.shape[:2] for m in members) or not _group_shapes_ok([(m[0], m[3], m[5]) for m in members]):
            return False
        descs = []
        for x_all, h0, c0, weight, bias, Hd, Cx in members:
            T, B, H, W, Cxp = x_all.shape
            pd = lstm_pack_desc(Hd, Cx, 3)
            # the step's descriptor with the right shapes (the planner does not dereference the pointers): x_t, h, panel geometry
            descs.append(_lstm_desc(*(None,) * 8, 3, probe=(B, H, W, (Cxp, Hd), pd.N, pd.Ktot, x_all.data_ptr()))[0])
        return group_launchable(descs)
    except Exception:
        return False


# ---------------------------------------------------------------------------------------------
# Loss (main.py:28-72)
# ---------------------------------------------------------------------------------------------
_LOSS_POINTS = {"l1": L.LOSS_POINT_L1, "l2": L.LOSS_POINT_L2, "huber": L.LOSS_POINT_HUBER}


def loss_spec_desc(spec) -> "L.LossSpecDesc":
    """uclstm_loss_spec of a loss.LossSpec: what the kernels read (grad_weight and eps stay on the host side)."""
    return L.LossSpecDesc(_LOSS_POINTS[spec.point], int(spec.weight_power), float(spec.delta), float(spec.weight_gain),
                          int(spec.grad_weight != 0))


def _mask_broadcast(y_pred, m) -> int:
    """Cy when the mask ``m`` has ONE channel (dim -3) where ``y_pred`` has Cy > 1 and all other dims agree; 1 otherwise."""
    if m is None or y_pred.dim() < 3 or m.dim() != y_pred.dim():
        return 1
    Cy = int(y_pred.shape[-3])
    if Cy > 1 and m.shape[-3] == 1 and m.shape[:-3] == y_pred.shape[:-3] and m.shape[-2:] == y_pred.shape[-2:]:
        return Cy
    return 1


# (frame_weights, channel_weights, T, Cy, device) -> (device f32 [T*Cy], the sum of that f32 table in f64).  Built once per key and
# never evicted (T*Cy*4 bytes each): no step and no graph capture after the first use holds a host-to-device copy, and the pointer a
# captured graph holds stays valid.
_PLANE_W = {}


def plane_weight_table(spec, y_pred):
    """The per-plane weights of a loss.WeightedLossSpec for ``y_pred [B,T,Cy,H,W]``: ``q[t*Cy + c] = f32(fw[t] * cw[c])``, the
    product formed in f64 and rounded once.  Returns ``(table on y_pred's device, sum(q) as a Python float)``."""
    if y_pred.dim() != 5:
        raise ValueError(f"a WeightedLossSpec with weights needs y_pred [B,T,Cy,H,W], got {y_pred.dim()} dimensions")
    T, Cy, dev = int(y_pred.shape[1]), int(y_pred.shape[2]), y_pred.device
    key = (spec.frame_weights, spec.channel_weights, T, Cy, dev.type, dev.index)
    hit = _PLANE_W.get(key)
    if hit is None:
        q = torch.tensor(spec.plane_weights(T, Cy), dtype=torch.float64).float()
        qsum = float(q.double().sum())
        if not qsum > 0:
            raise ValueError("WeightedLossSpec: every frame weight x channel weight product rounds to 0 in f32")
        hit = _PLANE_W[key] = (q.to(dev), qsum)
    return hit


class LossFn(torch.autograd.Function):
    """``spec``: None = the reference's loss on uclstm_loss_fwd / _bwd; a loss.LossSpec = uclstm_loss_spec_fwd / _bwd (loss.py
    sends the default spec here as None).  Both are logged as the reduction they are, loss_fwd / loss_fwd_ordered.
    A mask with ONE channel over a ``y`` of several (``y [B,T,Cy,H,W]``, ``mask [B,T,1,H,W]``: a vector target under the loaders'
    mask) is broadcast over the channels as main.py:40-43 does: uclstm_loss_spec_fwd_bc / _fwd_ordered_bc / _bwd_bc, where the
    reference's loss runs as ``LossSpec.reference()``.  Every other shape takes the entry points above.
    A loss.WeightedLossSpec with weights (``spec.weighted``) takes uclstm_loss_spec_fwd_pw / _fwd_ordered_pw / _bwd_pw with the
    cached table of plane_weight_table, whatever the mask's shape (mask_div = 1 for a mask per plane or none)."""

    @staticmethod
    def forward(ctx, y_pred, y, mask, use_mask, spec=None):
        _dev(y_pred, F32, "y_pred")
        y = _dev(y.contiguous(), F32, "y")
        H, W = y_pred.shape[-2], y_pred.shape[-1]
        planes = y_pred.numel() // (H * W)
        m = _dev(mask.contiguous().float(), F32, "mask") if (use_mask and mask is not None) else None
        desc = None if spec is None else loss_spec_desc(spec)
        # a one-channel mask over a target of Cy > 1 channels is broadcast (main.py:40-43, :64-66): the _bc entry points, on
        # which the reference's loss runs as its own LossSpec.  Every other shape keeps the entry points it always took.
        Cy = _mask_broadcast(y_pred, m)
        if Cy > 1 and desc is None:
            desc = L.LossSpecDesc(L.LOSS_POINT_L1, 3, 1.0, 4.0, 1)
        ctx.desc, ctx.mask_div, ctx.plane_w = desc, Cy, None
        if getattr(spec, "weighted", False):
            return LossFn._forward_pw(ctx, y_pred, y, m, spec, desc, Cy)
        if Cy > 1:
            return LossFn._forward_bc(ctx, y_pred, y, m, spec, desc, Cy)
        if _DETERMINISTIC:
            sums = torch.empty((4,), dtype=torch.float64, device=y_pred.device)
            partials = torch.empty((int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W)), 4), dtype=torch.float64, device=y_pred.device)
            _log_reduce("loss_fwd_ordered")
            if desc is None:
                L.check(L.lib.uclstm_loss_fwd_ordered(_p(y_pred), _p(y), _p(m), _p(partials), _p(sums), 0, planes, H, W, _stream()),
                        "loss_fwd_ordered")
            else:
                L.check(L.lib.uclstm_loss_spec_fwd_ordered(C.byref(desc), _p(y_pred), _p(y), _p(m), _p(partials), _p(sums), 0, planes, H, W,
                                                           _stream()), "loss_spec_fwd_ordered")
        else:
            sums = torch.zeros((4,), dtype=torch.float64, device=y_pred.device)
            _log_reduce("loss_fwd")
            if desc is None:
                L.check(L.lib.uclstm_loss_fwd(_p(y_pred), _p(y), _p(m), _p(sums), planes, H, W, _stream()), "loss_fwd")
            else:
                L.check(L.lib.uclstm_loss_spec_fwd(C.byref(desc), _p(y_pred), _p(y), _p(m), _p(sums), planes, H, W, _stream()),
                        "loss_spec_fwd")
        return LossFn._finish(ctx, y_pred, y, m, spec, sums)

    @staticmethod
    def _forward_bc(ctx, y_pred, y, m, spec, desc, Cy):
        H, W = y_pred.shape[-2], y_pred.shape[-1]
        planes = y_pred.numel() // (H * W)
        if _DETERMINISTIC:
            sums = torch.empty((4,), dtype=torch.float64, device=y_pred.device)
            partials = torch.empty((int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W)), 4), dtype=torch.float64, device=y_pred.device)
            _log_reduce("loss_fwd_ordered")
            L.check(L.lib.uclstm_loss_spec_fwd_ordered_bc(C.byref(desc), _p(y_pred), _p(y), _p(m), _p(partials), _p(sums), 0, planes, H, W,
                                                          Cy, _stream()), "loss_spec_fwd_ordered_bc")
        else:
            sums = torch.zeros((4,), dtype=torch.float64, device=y_pred.device)
            _log_reduce("loss_fwd")
            L.check(L.lib.uclstm_loss_spec_fwd_bc(C.byref(desc), _p(y_pred), _p(y), _p(m), _p(sums), planes, H, W, Cy, _stream()),
                    "loss_spec_fwd_bc")
        return LossFn._finish(ctx, y_pred, y, m, spec, sums)

    @staticmethod
    def _forward_pw(ctx, y_pred, y, m, spec, desc, mask_div):
        q, qsum = plane_weight_table(spec, y_pred)
        ctx.plane_w = q
        H, W = y_pred.shape[-2], y_pred.shape[-1]
        planes, period = y_pred.numel() // (H * W), q.numel()
        if _DETERMINISTIC:
            sums = torch.empty((4,), dtype=torch.float64, device=y_pred.device)
            partials = torch.empty((int(L.lib.uclstm_loss_fwd_ordered_rows(planes, H, W)), 4), dtype=torch.float64, device=y_pred.device)
            _log_reduce("loss_fwd_ordered")
            L.check(L.lib.uclstm_loss_spec_fwd_ordered_pw(C.byref(desc), _p(y_pred), _p(y), _p(m), _p(q), period, _p(partials), _p(sums), 0,
                                                          planes, H, W, mask_div, _stream()), "loss_spec_fwd_ordered_pw")
        else:
            sums = torch.zeros((4,), dtype=torch.float64, device=y_pred.device)
            _log_reduce("loss_fwd")
            L.check(L.lib.uclstm_loss_spec_fwd_pw(C.byref(desc), _p(y_pred), _p(y), _p(m), _p(q), period, _p(sums), planes, H, W, mask_div,
                                                  _stream()), "loss_spec_fwd_pw")
        # unmasked, every element of plane p counts q[p mod period] times: the denominators in f64 on the host, from the f32 table
        return LossFn._finish(ctx, y_pred, y, m, spec, sums, (planes // period) * qsum)

    @staticmethod
    def _finish(ctx, y_pred, y, m, spec, sums, plane_mass=None):
        """``plane_mass``: the summed weight of the planes (None: every plane counts once)."""
        H, W = y_pred.shape[-2], y_pred.shape[-1]
        planes = y_pred.numel() // (H * W)
        eps, gw = (1e-8, 0.005) if spec is None else (float(spec.eps), float(spec.grad_weight))
        n1 = float(y_pred.numel()) if plane_mass is None else float(H * W) * plane_mass
        n2 = float(planes * (H - 1) * (W - 1)) if plane_mass is None else float((H - 1) * (W - 1)) * plane_mass
        if m is not None:
            d1 = sums[1] + eps
            d2 = sums[3] + eps
        else:
            d1 = torch.full((), n1, dtype=torch.float64, device=y_pred.device)
            d2 = torch.full((), n2, dtype=torch.float64, device=y_pred.device)
        if gw == 0:                                                     # the gradient term does not exist (no 0 / 0 of an empty crop)
            loss = (sums[0] / d1).float()
            c2 = torch.zeros((), dtype=torch.float32, device=y_pred.device)
        else:
            loss = (sums[0] / d1 + gw * sums[2] / d2).float()
            c2 = (gw / d2).float()
        ctx.save_for_backward(y_pred, y, m, (1.0 / d1).float(), c2)
        return loss

    @staticmethod
    def backward(ctx, g):
        y_pred, y, m, c1, c2 = ctx.saved_tensors
        H, W = y_pred.shape[-2], y_pred.shape[-1]
        planes = y_pred.numel() // (H * W)
        grad = torch.empty_like(y_pred)
        coefs = torch.stack((c1 * g, c2 * g)).float().contiguous()      # stays on device: no host sync in the step
        if ctx.plane_w is not None:
            q = ctx.plane_w
            L.check(L.lib.uclstm_loss_spec_bwd_pw(C.byref(ctx.desc), _p(y_pred), _p(y), _p(m), _p(q), q.numel(), _p(coefs), _p(grad), planes,
                                                  H, W, ctx.mask_div, _stream()), "loss_spec_bwd_pw")
        elif ctx.mask_div > 1:
            L.check(L.lib.uclstm_loss_spec_bwd_bc(C.byref(ctx.desc), _p(y_pred), _p(y), _p(m), _p(coefs), _p(grad), planes, H, W,
                                                  ctx.mask_div, _stream()), "loss_spec_bwd_bc")
        elif ctx.desc is None:
            L.check(L.lib.uclstm_loss_bwd(_p(y_pred), _p(y), _p(m), _p(coefs), _p(grad), planes, H, W, _stream()), "loss_bwd")
        else:
            L.check(L.lib.uclstm_loss_spec_bwd(C.byref(ctx.desc), _p(y_pred), _p(y), _p(m), _p(coefs), _p(grad), planes, H, W, _stream()),
                    "loss_spec_bwd")
        return grad, None, None, None, None
