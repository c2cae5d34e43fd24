"""unet-convlstm_amd: the UNet-ConvLSTM training path of dordanino12/unet-convlstm on MI355X (gfx950).

Hand-written HIP kernels (libuclstm.so, C ABI in include/uclstm.h) behind the reference's own
nn.Module surface.  Importing this package loads the shared library and fails loudly if it is
missing -- there is no CPU or eager-PyTorch fallback for the compute path.

The directory name contains a hyphen (it mirrors the reference repository's name); import it as
``import unet_convlstm_amd`` (top-level alias module) or ``importlib.import_module("unet-convlstm_amd")``.
"""
from . import _lib
from ._lib import UclstmError
from . import ops
from .modules import (ConvLSTMCell, ConvLSTM, DoubleConv, Down, Up, OutConv, SpatialAttention,
                      TemporalUNetDualView, UNet)
from .resnet import PretrainedTemporalUNet
from .loss import compute_loss, LossSpec, WeightedLossSpec
from .optim import FusedAdamW, WeightEMA, StepMonitor
from .engine import train_one_epoch, evaluate, train_step, GraphedTrainStep, quiesce_host_gc, SyntheticSequences, NPZSequenceDataset, device_transform, EvalReport, evaluate_report, DeviceSequenceLoader, epoch_rows, Augment, epoch_augment, plane_d4, predict_tta, d4_inverse
from .engine import (DeviceSpriteLoader, render_sprites_host, epoch_sprites, check_sprite_table, load_idx_images,
                     procedural_glyphs)
from .engine import VectorNPZDataset, plane_d4_vec, VectorEvalReport, evaluate_vector_report
from .engine import DeviceNPZDataset, device_order_statistics, device_percentile, device_extremes, percentile_ranks, percentile_lerp
from .ddp import FlatDDP
from .streaming import StreamingPredictor, PretrainedStreamingPredictor
from .ops import compute_dtype, set_compute_dtype, get_compute_dtype
from .ops import deterministic, set_deterministic, is_deterministic
from .ops import sync_batchnorm, set_sync_batchnorm, get_sync_batchnorm

__all__ = ["ConvLSTMCell", "ConvLSTM", "DoubleConv", "Down", "Up", "OutConv", "SpatialAttention",
           "TemporalUNetDualView", "UNet", "PretrainedTemporalUNet", "compute_loss", "LossSpec", "WeightedLossSpec", "FusedAdamW", "WeightEMA", "StepMonitor", "train_one_epoch", "evaluate",
           "train_step", "GraphedTrainStep", "quiesce_host_gc", "SyntheticSequences", "NPZSequenceDataset", "device_transform", "EvalReport", "evaluate_report", "DeviceSequenceLoader", "epoch_rows", "Augment", "epoch_augment", "plane_d4", "predict_tta", "d4_inverse", "DeviceSpriteLoader", "render_sprites_host", "epoch_sprites", "check_sprite_table",
           "load_idx_images", "procedural_glyphs", "VectorNPZDataset", "plane_d4_vec", "VectorEvalReport", "evaluate_vector_report", "DeviceNPZDataset", "device_order_statistics", "device_percentile", "device_extremes",
           "percentile_ranks", "percentile_lerp", "FlatDDP", "StreamingPredictor", "PretrainedStreamingPredictor", "UclstmError", "ops",
           "compute_dtype", "set_compute_dtype", "get_compute_dtype", "deterministic", "set_deterministic", "is_deterministic",
           "sync_batchnorm", "set_sync_batchnorm", "get_sync_batchnorm"]
