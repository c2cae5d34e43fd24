"""ctypes binding of libuclstm.so (include/uclstm.h).

This is the only place the shared library is loaded.  There is no fallback: if the library is
missing or lacks a symbol the import of the product package fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import re

# PyTorch-ROCm bundles its own libamdhip64.so.7; libuclstm.so NEEDs the same SONAME.  torch must be loaded FIRST so that
# the dynamic linker resolves our dependency to the runtime torch already uses -- otherwise the process holds two HIP
# runtimes and launches on torch's device pointers fail with "no ROCm-capable device is detected".
import torch  # noqa: F401  (load order matters, see above)

HERE = os.path.dirname(os.path.abspath(__file__))
# UCLSTM_LIB: another build of the same library (same-box A/B timing of kernel variants); it must exist and match the ABI
LIB_PATH = os.environ.get("UCLSTM_LIB") or os.path.join(HERE, "libuclstm.so")
HEADER_PATH = os.path.join(HERE, "..", "include", "uclstm.h")

ABI_VERSION = 16
EPI_STORE, EPI_LSTM, EPI_ATOMIC = 0, 1, 2
NMODE_IDENTITY, NMODE_LSTM, NMODE_TAPMAJOR = 0, 1, 2
KMODE_IDENTITY, KMODE_GATES, KMODE_IM2COL = 0, 1, 2
ACT_TYPE_BF16, ACT_TYPE_F16 = 0, 1

_ERRORS = {-1: "bad argument (shape/alignment/null contract)", -2: "kernel launch failed", -3: "no gfx950 device"}


class UclstmError(RuntimeError):
    pass


class Src(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("C", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32),
                ("offY", C.c_int32), ("offX", C.c_int32)]


class Seg(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("n_begin", C.c_int32), ("n_end", C.c_int32), ("C", C.c_int32),
                ("c_off", C.c_int32), ("Hd", C.c_int32), ("Wd", C.c_int32), ("scale", C.c_int32),
                ("oy", C.c_int32), ("ox", C.c_int32)]


class IgemmDesc(C.Structure):
    _fields_ = [("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("groups", C.c_int32),
                ("ktap", C.c_int32), ("scale", C.c_int32), ("pad", C.c_int32), ("nsrc", C.c_int32),
                ("src", Src * 2),
                ("wp", C.c_void_p), ("N", C.c_int32), ("Ktot", C.c_int32),
                ("bias", C.c_void_p), ("col_scale", C.c_void_p), ("col_shift", C.c_void_p),
                ("relu", C.c_int32), ("epi", C.c_int32),
                ("nseg", C.c_int32), ("seg", Seg * 4),
                ("stats", C.c_void_p),
                ("Hd_p", C.c_int32), ("c_prev", C.c_void_p), ("c_out", C.c_void_p), ("h_out", C.c_void_p),
                ("gates_out", C.c_void_p), ("pre_add", C.c_void_p),
                ("acc_out", C.c_void_p), ("acc_ld", C.c_int32), ("ksplit", C.c_int32), ("acc_slab", C.c_int64)]


class WgradDesc(C.Structure):
    _fields_ = [("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("ktap", C.c_int32), ("scale", C.c_int32), ("pad", C.c_int32), ("nsrc", C.c_int32),
                ("src", Src * 2),
                ("N", C.c_int32), ("Ktot", C.c_int32),
                ("nseg", C.c_int32), ("seg", Seg * 4),
                ("dwp", C.c_void_p), ("splits", C.c_int32), ("accumulate", C.c_int32), ("overlapped", C.c_int32), ("reserved_", C.c_int32),
                ("slab", C.c_int64)]


class LstmFwdPwArgs(C.Structure):
    _fields_ = [("pre", C.c_void_p), ("pre_add", C.c_void_p), ("bias", C.c_void_p), ("c_prev", C.c_void_p), ("c_out", C.c_void_p),
                ("h_out", C.c_void_p), ("gates_out", C.c_void_p), ("slab", C.c_int64), ("pixels", C.c_int64),
                ("nslab", C.c_int32), ("clear", C.c_int32), ("Hd_p", C.c_int32), ("reserved_", C.c_int32)]


class PackDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("Ktot", C.c_int32), ("taps", C.c_int32), ("nsrc", C.c_int32),
                ("kseg", C.c_int32 * 2), ("cvalid", C.c_int32 * 2), ("choff", C.c_int32 * 2),
                ("n_mode", C.c_int32), ("n_valid", C.c_int32), ("n_cp", C.c_int32),
                ("k_mode", C.c_int32), ("k_hdp", C.c_int32), ("k_hd", C.c_int32),
                ("tap_flip", C.c_int32),
                ("stride_n", C.c_int64), ("stride_k", C.c_int64), ("stride_tap", C.c_int64),
                ("stride_ntap", C.c_int64)]


class PackJob(C.Structure):
    _fields_ = [("d", PackDesc), ("w", C.c_void_p), ("wp", C.c_void_p),
                ("block0", C.c_int32), ("nblocks", C.c_int32), ("gx", C.c_int32), ("family", C.c_int32),
                ("div", C.c_uint32 * 15), ("pad_", C.c_int32)]


class EvalDesc(C.Structure):
    _fields_ = [("y_pred", C.c_void_p), ("pred_stride_b", C.c_int64), ("pred_stride_t", C.c_int64),
                ("y", C.c_void_p), ("y_stride_b", C.c_int64), ("y_stride_t", C.c_int64),
                ("mask", C.c_void_p), ("mask_stride_b", C.c_int64), ("mask_stride_t", C.c_int64),
                ("B", C.c_int32), ("T", C.c_int32), ("P", C.c_int64),
                ("transform", C.c_int32), ("y_scale", C.c_float), ("trans_min", C.c_float), ("trans_max", C.c_float),
                ("table", C.c_void_p), ("bins", C.c_int32), ("n_edges", C.c_int32),
                ("hist_lo", C.c_double), ("hist_hi", C.c_double), ("err_lo", C.c_double), ("err_hi", C.c_double),
                ("dig_lo", C.c_double), ("dig_w", C.c_double),
                ("hist", C.c_void_p), ("dig_count", C.c_void_p), ("scatter", C.c_void_p),
                ("seed", C.c_uint64), ("K", C.c_int32), ("reserved_", C.c_int32)]


class LossSpecDesc(C.Structure):
    """uclstm_loss_spec: host memory, read at launch (grad_weight and eps of loss.LossSpec stay on the host side)."""
    _fields_ = [("point", C.c_int32), ("weight_power", C.c_int32), ("delta", C.c_float), ("weight_gain", C.c_float),
                ("grad_term", C.c_int32), ("reserved_", C.c_int32 * 3)]


class SelectState(C.Structure):
    """uclstm_select_state: host memory, written by the uclstm_select_* calls only."""
    _fields_ = [("workspace", C.c_void_p), ("n_slots", C.c_int32), ("abs_mask", C.c_uint32), ("phase", C.c_int32), ("magic", C.c_uint32)]


class TargetConsts(C.Structure):
    """uclstm_target_consts: the normalisation constants of ONE target channel; arrays of it live in host memory, read at launch."""
    _fields_ = [("min_vel", C.c_float), ("max_vel", C.c_float), ("y_scale", C.c_float), ("trans_min", C.c_float), ("trans_max", C.c_float)]


class EvalVecDesc(C.Structure):
    """uclstm_eval_vec_desc: the report of uclstm_eval_stats for frames of Cy target channels, per-channel fields as arrays of VEC_MAX."""
    _fields_ = [("y_pred", C.c_void_p), ("pred_stride_b", C.c_int64), ("pred_stride_t", C.c_int64),
                ("y", C.c_void_p), ("y_stride_b", C.c_int64), ("y_stride_t", C.c_int64),
                ("mask", C.c_void_p), ("mask_stride_b", C.c_int64), ("mask_stride_t", C.c_int64),
                ("B", C.c_int32), ("T", C.c_int32), ("Cy", C.c_int32), ("transform", C.c_int32), ("HW", C.c_int64),
                ("consts", TargetConsts * 4),
                ("hist_lo", C.c_double * 4), ("hist_hi", C.c_double * 4), ("err_lo", C.c_double * 4), ("err_hi", C.c_double * 4),
                ("dig_lo", C.c_double * 4), ("dig_w", C.c_double * 4),
                ("bins", C.c_int32), ("n_edges", C.c_int32), ("K", C.c_int32), ("dir_bins", C.c_int32),
                ("seed", C.c_uint64),
                ("w_chan", C.c_int32), ("h_chan", C.c_int32), ("w_sign", C.c_int32), ("h_sign", C.c_int32),
                ("speed_hi", C.c_double), ("epe_hi", C.c_double), ("min_speed", C.c_double),
                ("table", C.c_void_p), ("hist", C.c_void_p), ("dig_count", C.c_void_p), ("scatter", C.c_void_p),
                ("vtable", C.c_void_p), ("vhist", C.c_void_p), ("dir_hist", C.c_void_p)]


LOSS_POINT_L1, LOSS_POINT_L2, LOSS_POINT_HUBER = 0, 1, 2
VEC_MAX = 4                  # UCLSTM_VEC_MAX: target channels of the vector data path
SELECT_MAX_SLOTS, SELECT_BINS, SELECT_SIGNED, SELECT_ABS = 8, 2048, 0, 1
SELECT_WS_COUNT, SELECT_WS_NAN, SELECT_WS_FLAGS, SELECT_WS_PREFIX, SELECT_WS_RANK, SELECT_WS_LEADER, SELECT_WS_HIST = 0, 1, 2, 8, 16, 24, 32
EXTREMES_MIN_KEY, EXTREMES_MAX_KEY, EXTREMES_NAN, EXTREMES_NONZERO, EXTREMES_COUNT, EXTREMES_WORDS = 0, 1, 2, 3, 4, 8
EVAL_ROW = 16
EVAL_VROW = 16               # UCLSTM_EVAL_VROW: doubles per row of the vector table
EVAL_NONE, EVAL_ASINH, EVAL_SIGNED_LOG = 0, 1, 2

_P, _I, _L, _F = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name -> argtypes (restype int32 unless listed in _RESTYPES)
_PROTOS = {
    "uclstm_igemm_tiles_per_group": [_I, _I, _I, _I, _I],
    "uclstm_igemm_fwd": [C.POINTER(IgemmDesc), _P],
    "uclstm_igemm_fwd_shape": [_P],
    "uclstm_igemm_ksplit_used": [_I, _I, _I],
    "uclstm_igemm_fwd_group": [C.POINTER(IgemmDesc), _I, _P],
    "uclstm_igemm_fwd_group_blocks": [C.POINTER(IgemmDesc), _I],
    "uclstm_igemm_fwd_group_tap": [C.POINTER(IgemmDesc), _I, _P],
    "uclstm_igemm_fwd_group_tap_blocks": [C.POINTER(IgemmDesc), _I],
    "uclstm_igemm_wgrad": [C.POINTER(WgradDesc), _P],
    "uclstm_igemm_wgrad_splits": [C.POINTER(WgradDesc)],
    "uclstm_igemm_wgrad_shape": [C.POINTER(WgradDesc)],
    "uclstm_igemm_wgrad_walk": [C.POINTER(WgradDesc), _I, _L, _I, C.POINTER(C.c_int32)],
    "uclstm_pack_weights": [C.POINTER(PackDesc), _P, _P, _P],
    "uclstm_pack_job_init": [C.POINTER(PackJob), C.POINTER(PackDesc), _P, _P, _I],
    "uclstm_pack_weights_batched": [_P, _I, _I, _I, _P],
    "uclstm_unpack_wgrad": [C.POINTER(PackDesc), _P, _I, _L, _P, _I, _P],
    "uclstm_unpack_wgrad_ordered_groups": [C.POINTER(PackDesc), _I],
    "uclstm_unpack_wgrad_ordered": [C.POINTER(PackDesc), _P, _I, _L, _P, _P, _I, _P],
    "uclstm_pack_bias": [C.POINTER(PackDesc), _P, _P, _P],
    "uclstm_bn_finalize": [_P, _I, _I, _I, _I, _L, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P],
    "uclstm_bn_stats_fwd": [_P, _I, _I, _I, _I, _L, _P, _P, _F, _P, _P, _P, _P, _P],
    "uclstm_bn_running_stats": [_P, _I, _I, _I, _I, _L, _P, _P, _F, _P],
    "uclstm_bn_stats_partial": [_P, _I, _I, _I, _P, _P],
    "uclstm_bn_stats_from_sums": [_P, _L, _P, _I, _I, _I, _I, _P, _P, _F, _P, _P, _P, _P, _P],
    "uclstm_bn_bwd_sums_stage": [_P, _P, _L, _P],
    "uclstm_bn_bwd_sums_finish": [_P, C.c_double, _P, _L, _P],
    "uclstm_bn_apply_relu": [_P, _P, _P, _P, _L, _L, _I, _P],
    "uclstm_bn_bwd_reduce_rows": [_L, _L],
    "uclstm_bn_bwd_reduce": [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P],
    "uclstm_bn_bwd_apply": [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P],
    "uclstm_bn_pool_bwd_rows": [_L, _I, _I, _I, _I],
    "uclstm_bn_apply_relu_pool": [_P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "uclstm_bn_pool_bwd_reduce": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "uclstm_bn_pool_bwd_apply": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "uclstm_bn_head_fwd": [_P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _P],
    "uclstm_bn_head_bwd_reduce": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _P],
    "uclstm_bn_head_bwd_reduce_ordered": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _I, _P],
    "uclstm_bn_head_bwd_apply": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _P],
    "uclstm_bn_bwd_param_grads": [_P, _I, _I, _I, _P, _P, _I, _P],
    "uclstm_maxpool2_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "uclstm_maxpool2_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "uclstm_lstm_bwd_pointwise": [_P, _P, _P, _P, _P, _I, _I, _L, _P, _I, _P, _L, _I, _P],
    "uclstm_lstm_fwd_pointwise": [_P, _I, _L, _I, _P, _P, _P, _P, _P, _P, _L, _I, _P],
    "uclstm_lstm_fwd_pointwise_group": [C.POINTER(LstmFwdPwArgs), _I, _P],
    "uclstm_splitk_finish": [_P, _I, _L, _I, _P, _P, _P, _I, _P, _L, _I, _P],
    "uclstm_nchw_to_nhwc": [_P, _P, _I, _I, _I, _I, _I, _I, _L, _L, _P],
    "uclstm_nhwc_to_nchw": [_P, _P, _I, _I, _I, _I, _I, _P],
    "uclstm_nchw_grad_to_nhwc": [_P, _P, _I, _I, _I, _I, _I, _P],
    "uclstm_im2col3x3_first": [_P, _P, _I, _I, _I, _I, _I, _I, _L, _L, _P],
    "uclstm_nchw_to_nhwc_f32": [_P, _P, _I, _I, _I, _I, _I, _P],
    "uclstm_nhwc_to_nchw_f32": [_P, _P, _I, _I, _I, _I, _I, _P],
    "uclstm_outconv_fwd": [_P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "uclstm_outconv_bwd": [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "uclstm_outconv_bwd_ordered_rows": [_L, _I],
    "uclstm_outconv_bwd_ordered": [_P, _P, _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _I, _I, _P],
    "uclstm_im2col7x7s2_first": [_P, _P, _I, _I, _I, _I, _I, _I, _L, _L, _P],
    "uclstm_maxpool3s2_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "uclstm_bn_add_relu": [_P, _P, _P, _P, _P, _P, _P, _L, _I, _P],
    "uclstm_upsample2_fwd": [_P, _P, _I, _I, _I, _I, _P],
    "uclstm_upsample2_bwd": [_P, _P, _I, _I, _I, _I, _P],
    "uclstm_head3x3_fwd": [_P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    "uclstm_head3x3_bwd": [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    "uclstm_head3x3_bwd_ordered_rows": [_L, _I, _I],
    "uclstm_head3x3_bwd_ordered": [_P, _P, _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _I, _I, _I, _P],
    "uclstm_maxpool3s2_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "uclstm_bn_add_relu_bwd_rows": [_L],
    "uclstm_bn_add_relu_bwd_reduce": [_P] * 14 + [_L, _I, _P],
    "uclstm_bn_add_relu_bwd_apply": [_P] * 15 + [_L, _I, _P],
    "uclstm_colsum": [_P, _P, _L, _I, _P],
    "uclstm_colsum_ordered_rows": [_L, _I],
    "uclstm_colsum_ordered": [_P, _P, _P, _L, _I, _I, _I, _P],
    "uclstm_ordered_sum_f32": [_P, _I, _I, _P, _I, _P],
    "uclstm_ordered_sum_f64": [_P, _I, _I, _P, _I, _P],
    "uclstm_attention_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "uclstm_attention_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P],
    "uclstm_loss_fwd": [_P, _P, _P, _P, _L, _I, _I, _P],
    "uclstm_loss_fwd_ordered_rows": [_L, _I, _I],
    "uclstm_loss_fwd_ordered": [_P, _P, _P, _P, _P, _I, _L, _I, _I, _P],
    "uclstm_loss_bwd": [_P, _P, _P, _P, _P, _L, _I, _I, _P],
    "uclstm_loss_spec_fwd": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _L, _I, _I, _P],
    "uclstm_loss_spec_fwd_ordered": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _P, _I, _L, _I, _I, _P],
    "uclstm_loss_spec_bwd": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _P, _L, _I, _I, _P],
    "uclstm_loss_spec_fwd_bc": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _L, _I, _I, _I, _P],
    "uclstm_loss_spec_fwd_ordered_bc": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _P],
    "uclstm_loss_spec_bwd_bc": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _P, _L, _I, _I, _I, _P],
    "uclstm_loss_spec_fwd_pw": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _I, _P, _L, _I, _I, _I, _P],
    "uclstm_loss_spec_fwd_ordered_pw": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _I, _P, _P, _I, _L, _I, _I, _I, _P],
    "uclstm_loss_spec_bwd_pw": [C.POINTER(LossSpecDesc), _P, _P, _P, _P, _I, _P, _P, _L, _I, _I, _I, _P],
    "uclstm_sumsq": [_P, _L, _P, _P],
    "uclstm_sumsq_ordered_rows": [_L],
    "uclstm_sumsq_ordered": [_P, _L, _P, _P, _I, _P],
    "uclstm_adamw_step": [_P, _P, _P, _P, _L, _P, _F, _F, _F, _F, _F, _F, _I, _P],
    "uclstm_adamw_step_dev": [_P, _P, _P, _P, _L, _P, _P, _P],
    "uclstm_adamw_step_groups": [_P, _P, _P, _P, _L, _P, _P, _I, _P, _I, _P, _P],
    "uclstm_adamw_step_scaled": [_P, _P, _P, _P, _L, _P, _F, _F, _F, _F, _F, _F, _P, _P],
    "uclstm_loss_scale_update": [_P, _P, _F, _F, _I, _P],
    "uclstm_ema_update": [_P, _P, _L, _P, _P, _P],
    "uclstm_swap_f32": [_P, _P, _L, _P],
    "uclstm_param_stats_chunk": [],
    "uclstm_param_stats": [_P, _P, _P, _L, _P, _L, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P],
    "uclstm_dataset_transform": [_P, _P, _P, _P, _P, _L, _I, _I, _F, _F, _F, _I, _F, _F, _F, _P],
    "uclstm_dataset_gather_transform": [_P, _P, _P, _L, _L, _I, _I, _I, _P, _P, _P, _I, _F, _F, _F, _I, _F, _F, _F, _P],
    "uclstm_dataset_gather_augment": [_P, _P, _P, _P, _L, _L, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _F, _F, _F, _I, _F, _F, _F, _P],
    "uclstm_plane_d4": [_P, _P, _L, _I, _I, _I, _I, _F, _P],
    "uclstm_dataset_gather_vec": [_P, _P, _P, _P, _L, _L, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _F, _I, C.POINTER(TargetConsts), _P],
    "uclstm_plane_d4_vec": [_P, _P, _L, _I, _I, _I, _I, _P, _P, _I, _F, _P],
    "uclstm_sprites_render": [_P, _I, _I, _I, _P, _L, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P],
    "uclstm_metric_sums": [_P, _P, _P, _P, _L, _F, _F, _F, _P],
    "uclstm_metric_sums_ordered_rows": [_L],
    "uclstm_metric_sums_ordered": [_P, _P, _P, _P, _P, _I, _L, _F, _F, _F, _P],
    "uclstm_metric_sums_vec_rows": [_L, _I, _I],
    "uclstm_metric_sums_vec": [_P, _P, _P, _P, _P, _I, _L, _I, _I, _I, C.POINTER(TargetConsts), _P],
    "uclstm_eval_stats": [C.POINTER(EvalDesc), _P],
    "uclstm_eval_stats_rows": [_L, _L],
    "uclstm_eval_stats_vec": [C.POINTER(EvalVecDesc), _P],
    "uclstm_select_workspace_bytes": [],
    "uclstm_select_begin": [C.POINTER(SelectState), _P, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _I, _P],
    "uclstm_select_accumulate": [C.POINTER(SelectState), _I, _P, _L, _P],
    "uclstm_select_narrow": [C.POINTER(SelectState), _I, _P],
    "uclstm_select_finish": [C.POINTER(SelectState), _P, _P, _P],
    "uclstm_dataset_extremes_begin": [_P, _P],
    "uclstm_dataset_extremes": [_P, _L, _P, _P],
    "uclstm_stream_spin": [_I, _P],
    "uclstm_abi_version": [],
    "uclstm_build_arch": [],
    "uclstm_source_hash": [],
    "uclstm_last_error_string": [],
}
_RESTYPES = {"uclstm_igemm_wgrad_walk": C.c_int64, "uclstm_build_arch": C.c_char_p, "uclstm_source_hash": C.c_char_p, "uclstm_last_error_string": C.c_char_p, "uclstm_bn_bwd_reduce_rows": C.c_int64, "uclstm_bn_pool_bwd_rows": C.c_int64,
             "uclstm_eval_stats_rows": C.c_int64, "uclstm_colsum_ordered_rows": C.c_int64, "uclstm_outconv_bwd_ordered_rows": C.c_int64, "uclstm_head3x3_bwd_ordered_rows": C.c_int64,
             "uclstm_loss_fwd_ordered_rows": C.c_int64, "uclstm_sumsq_ordered_rows": C.c_int64, "uclstm_metric_sums_ordered_rows": C.c_int64, "uclstm_metric_sums_vec_rows": C.c_int64,
             "uclstm_bn_add_relu_bwd_rows": C.c_int64, "uclstm_select_workspace_bytes": C.c_int64,
             "uclstm_param_stats_chunk": C.c_int64}


# entry points that exist twice: name (bfloat16) and name_f16 (IEEE binary16), identical signatures (include/uclstm.h)
F16_TWINS = ['uclstm_igemm_fwd', 'uclstm_igemm_fwd_group', 'uclstm_igemm_wgrad', 'uclstm_pack_weights', 'uclstm_pack_weights_batched', 'uclstm_bn_apply_relu', 'uclstm_bn_bwd_reduce', 'uclstm_bn_bwd_apply', 'uclstm_bn_apply_relu_pool', 'uclstm_bn_pool_bwd_reduce', 'uclstm_bn_pool_bwd_apply', 'uclstm_bn_head_fwd', 'uclstm_bn_head_bwd_reduce', 'uclstm_bn_head_bwd_apply', 'uclstm_maxpool2_fwd', 'uclstm_maxpool2_bwd', 'uclstm_lstm_bwd_pointwise', 'uclstm_lstm_fwd_pointwise', 'uclstm_lstm_fwd_pointwise_group', 'uclstm_splitk_finish', 'uclstm_nchw_to_nhwc', 'uclstm_nhwc_to_nchw', 'uclstm_nchw_grad_to_nhwc', 'uclstm_im2col3x3_first', 'uclstm_outconv_fwd', 'uclstm_outconv_bwd', 'uclstm_colsum', 'uclstm_attention_fwd', 'uclstm_attention_bwd']
# the twins of csrc/resnet.hip (the ResNet18-encoder model), declared in the header as one list (UCLSTM_RESNET_F16_TWINS) and kept
# as a list of their own here (tests/test_cabi_and_host.py and three more pin the list above at its 29 entries): bound, resolved
# and exported exactly like the ones above
RESNET_F16_TWINS = ['uclstm_im2col7x7s2_first', 'uclstm_maxpool3s2_fwd', 'uclstm_bn_add_relu', 'uclstm_upsample2_fwd', 'uclstm_upsample2_bwd',
                    'uclstm_head3x3_fwd', 'uclstm_head3x3_bwd']
# the twins of csrc/resnet_bwd.hip (training the encoder), the header's UCLSTM_RESNET_BWD_F16_TWINS: a list of their own for the same reason
RESNET_BWD_F16_TWINS = ['uclstm_maxpool3s2_bwd', 'uclstm_bn_add_relu_bwd_reduce', 'uclstm_bn_add_relu_bwd_apply']
# the twin of the per-tap group launch (csrc/igemm_fwd.hip), the header's UCLSTM_TAP_GROUP_F16_TWINS: a list of its own for the same reason
TAP_GROUP_F16_TWINS = ['uclstm_igemm_fwd_group_tap']
_ALL_F16_TWINS = frozenset(F16_TWINS) | frozenset(RESNET_F16_TWINS) | frozenset(RESNET_BWD_F16_TWINS) | frozenset(TAP_GROUP_F16_TWINS)


def header_symbols() -> list[str]:
    """Every function name declared in include/uclstm.h (the fp16 twins are declared through UCLSTM_F16_TWIN(name))."""
    with open(HEADER_PATH) as f:
        text = f.read()
    names = set(re.findall(r"\b(uclstm_[a-z0-9_]+)\s*\(", text))
    names |= {n + "_f16" for n in re.findall(r"^UCLSTM_F16_TWIN\((uclstm_[a-z0-9_]+)\)", text, re.M)}
    return sorted(names)


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise UclstmError(
            f"{LIB_PATH} is missing: build it with `python unet-convlstm_amd/build.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for this package.")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in list(_PROTOS.items()):
        for sym in ([name, name + "_f16"] if name in _ALL_F16_TWINS else [name]):
            try:
                fn = getattr(lib, sym)
            except AttributeError as e:
                raise UclstmError(f"{LIB_PATH} does not export {sym}; rebuild the library") from e
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int32)
    if lib.uclstm_abi_version() != ABI_VERSION:
        raise UclstmError("libuclstm.so ABI version mismatch; rebuild the library")
    if not os.environ.get("UCLSTM_LIB"):
        # ship exactly what is tracked: the library says which sources it was built from (build.py: source_hash)
        from . import build as _build
        built, tree = lib.uclstm_source_hash().decode(), _build.source_hash()
        if built != tree:
            raise UclstmError(f"{LIB_PATH} was built from other sources than this tree (library {built[:16]}, tree {tree[:16]}): "
                              "run `python unet-convlstm_amd/build.py`")
    return lib


lib = _load()


class _F16Kernels:
    """The same entry points for IEEE binary16 activations: twins resolve to ``name_f16``, shared ones to ``name``."""

    def __getattr__(self, name):
        fn = getattr(lib, name + "_f16" if name in _ALL_F16_TWINS else name)
        setattr(self, name, fn)
        return fn


lib16 = _F16Kernels()


def kernels(dtype):
    """Kernel set for a 16-bit activation dtype: ``torch.bfloat16`` -> ``lib``, ``torch.float16`` -> ``lib16``."""
    if dtype == torch.bfloat16:
        return lib
    if dtype == torch.float16:
        return lib16
    raise UclstmError(f"activations must be torch.bfloat16 or torch.float16, got {dtype}")


def act_type(dtype) -> int:
    """``act_type`` argument of the entry points that read 16-bit activations but exist once (the ordered reductions)."""
    if dtype == torch.bfloat16:
        return ACT_TYPE_BF16
    if dtype == torch.float16:
        return ACT_TYPE_F16
    raise UclstmError(f"activations must be torch.bfloat16 or torch.float16, got {dtype}")


def check(rc: int, what: str) -> None:
    if rc != 0:
        detail = f" [{lib.uclstm_last_error_string().decode()}]" if rc == -2 else ""
        raise UclstmError(f"{what}: {_ERRORS.get(rc, 'error')} (code {rc}){detail}")
