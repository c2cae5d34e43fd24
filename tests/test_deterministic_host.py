"""Deterministic mode, the part that needs no GPU: the ordered entry points are declared, bound and exported consistently (and
the ABI version and the fp16-twin list did not move), the row / group planners are functions of shapes alone inside their
stated range, and the switch behaves like the package's other switches.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd import ops

ROWS_CAP = 1024

ORDERED = ["uclstm_colsum_ordered", "uclstm_colsum_ordered_rows", "uclstm_outconv_bwd_ordered", "uclstm_outconv_bwd_ordered_rows",
           "uclstm_bn_head_bwd_reduce_ordered", "uclstm_unpack_wgrad_ordered", "uclstm_unpack_wgrad_ordered_groups",
           "uclstm_loss_fwd_ordered", "uclstm_loss_fwd_ordered_rows", "uclstm_sumsq_ordered", "uclstm_sumsq_ordered_rows",
           "uclstm_metric_sums_ordered", "uclstm_metric_sums_ordered_rows", "uclstm_ordered_sum_f32", "uclstm_ordered_sum_f64"]


def test_header_binding_and_library_agree_on_the_ordered_entry_points():
    syms = set(L.header_symbols())
    raw = C.CDLL(L.LIB_PATH)
    for name in ORDERED:
        assert name in syms, f"{name} is not declared in include/uclstm.h"
        assert name in L._PROTOS, f"{name} has no ctypes prototype"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        # one symbol each: the activation type is an argument, not a twin
        assert name not in L.F16_TWINS and name + "_f16" not in syms and not hasattr(raw, name + "_f16")
    assert syms == set(L._PROTOS) | {n + "_f16" for n in L.F16_TWINS}
    for name in ORDERED:
        if name.endswith(("_rows",)):
            assert L._RESTYPES.get(name) is C.c_int64, name
    hdr = open(L.HEADER_PATH).read()
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16 == int(re.search(r"#define UCLSTM_ABI_VERSION (\d+)", hdr).group(1))
    assert len(L.F16_TWINS) == 29 and len(re.findall(r"^UCLSTM_F16_TWIN\(", hdr, re.M)) == 29
    assert (L.ACT_TYPE_BF16, L.ACT_TYPE_F16) == tuple(int(re.search(rf"#define UCLSTM_ACT_TYPE_{t}\s+(\d+)", hdr).group(1)) for t in ("BF16", "F16"))
    assert L.act_type(torch.bfloat16) == L.ACT_TYPE_BF16 and L.act_type(torch.float16) == L.ACT_TYPE_F16
    with pytest.raises(L.UclstmError):
        L.act_type(torch.float32)


def _monotone(values):
    return all(b >= a for a, b in zip(values, values[1:]))


SIZES = [1, 2, 3, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 4099, 20000, 65536, 262144, 262145, 1 << 20, (1 << 20) + 1, 1 << 24, 1 << 27]


def test_row_planners_depend_on_shapes_alone_and_stay_within_the_cap():
    lib = L.lib
    planners = {
        "colsum Cp=8": lambda n: lib.uclstm_colsum_ordered_rows(n, 8),
        "colsum Cp=72": lambda n: lib.uclstm_colsum_ordered_rows(n, 72),
        "colsum Cp=1024": lambda n: lib.uclstm_colsum_ordered_rows(n, 1024),
        "colsum Cp=4096": lambda n: lib.uclstm_colsum_ordered_rows(n, 4096),
        "outconv HW=1": lambda n: lib.uclstm_outconv_bwd_ordered_rows(n, 1),
        "outconv HW=323": lambda n: lib.uclstm_outconv_bwd_ordered_rows(n, 323),
        "loss 8x8": lambda n: lib.uclstm_loss_fwd_ordered_rows(min(n, (1 << 25) - 1), 8, 8),      # planes * H * W < 2^31
        "loss 1xn": lambda n: lib.uclstm_loss_fwd_ordered_rows(1, 1, n),
        "sumsq": lambda n: lib.uclstm_sumsq_ordered_rows(n),
        "metric sums": lambda n: lib.uclstm_metric_sums_ordered_rows(n),
    }
    for name, plan in planners.items():
        rows = [int(plan(n)) for n in SIZES]
        assert all(1 <= r <= ROWS_CAP for r in rows), (name, rows)
        assert _monotone(rows), (name, rows)
        assert rows == [int(plan(n)) for n in SIZES], name               # equal for equal shapes
        assert rows[0] == 1 and rows[-1] == ROWS_CAP, (name, rows)        # one block for one element, the cap at the far end
    # more channels per pixel -> fewer pixel rows per sweep -> never fewer rows
    for n in SIZES:
        assert _monotone([int(lib.uclstm_colsum_ordered_rows(n, cp)) for cp in (8, 16, 64, 256, 2048)])
    # the same plan as the launches they size: sumsq counts float4 quads, the loss and the metrics elements
    assert int(lib.uclstm_sumsq_ordered_rows(1025 * 4)) == 5 and int(lib.uclstm_metric_sums_ordered_rows(1025)) == 5
    assert int(lib.uclstm_loss_fwd_ordered_rows(3, 17, 19)) == (3 * 17 * 19 + 255) // 256
    # contract violations are codes, not launches
    assert lib.uclstm_colsum_ordered_rows(0, 8) == -1 and lib.uclstm_colsum_ordered_rows(5, 12) == -1
    assert lib.uclstm_outconv_bwd_ordered_rows(0, 4) == -1 and lib.uclstm_loss_fwd_ordered_rows(1, 0, 4) == -1
    assert lib.uclstm_sumsq_ordered_rows(0) == -1 and lib.uclstm_metric_sums_ordered_rows(-3) == -1


def test_unpack_group_planner_depends_on_descriptor_and_slab_count_alone():
    lib = L.lib
    first = ops.im2col_pack_desc(64, 1, 16)                       # first-layer-like: N * Ktot = 4096, not a row-family panel
    assert first.N * first.Ktot == 4096
    counts = [1, 2, 7, 15, 16, 17, 64, 65, 300, 1000, 4000, 100000]
    groups = [int(lib.uclstm_unpack_wgrad_ordered_groups(C.byref(first), n)) for n in counts]
    assert all(1 <= g <= ROWS_CAP for g in groups) and _monotone(groups), groups
    assert groups == [int(lib.uclstm_unpack_wgrad_ordered_groups(C.byref(first), n)) for n in counts]
    assert groups[:3] == [1, 1, 1] and groups[counts.index(300)] > 1
    for n, g in zip(counts, groups):
        assert g == 1 or (n + g - 1) // g >= 4                     # at least four slabs per group
    # a row-family panel is folded / unpacked by the ordered kernels the default path already has: one group at any count
    conv = ops.conv_pack_desc(40, 24, [24], [24])
    assert [int(lib.uclstm_unpack_wgrad_ordered_groups(C.byref(conv), n)) for n in counts] == [1] * len(counts)
    # more elements per slab -> the x grid alone fills the chip -> never more groups
    by_size = [int(lib.uclstm_unpack_wgrad_ordered_groups(C.byref(ops.im2col_pack_desc(co, 1, 16)), 300)) for co in (8, 64, 512, 4096)]
    assert _monotone(by_size[::-1]), by_size
    assert lib.uclstm_unpack_wgrad_ordered_groups(C.byref(first), 0) == -1
    # bad arguments are refused before any launch (no device is touched here)
    assert lib.uclstm_unpack_wgrad_ordered(C.byref(first), None, 300, 4096, None, None, 1, None) == -1
    assert lib.uclstm_colsum_ordered(None, None, None, 4, 8, 0, 0, None) == -1
    assert lib.uclstm_ordered_sum_f32(None, 1, 1, None, 0, None) == -1 and lib.uclstm_ordered_sum_f64(None, 1, 1, None, 0, None) == -1


def test_switch_is_exported_and_the_context_manager_restores_the_previous_value():
    assert U.set_deterministic is ops.set_deterministic and U.is_deterministic is ops.is_deterministic and U.deterministic is ops.deterministic
    for name in ("deterministic", "set_deterministic", "is_deterministic"):
        assert name in U.__all__
    start = ops.is_deterministic()
    try:
        ops.set_deterministic(False)
        with ops.deterministic():
            assert ops.is_deterministic()
            with ops.deterministic(False):
                assert not ops.is_deterministic()
                with ops.deterministic(True):
                    assert ops.is_deterministic()
                assert not ops.is_deterministic()
            assert ops.is_deterministic()
        assert not ops.is_deterministic()
        with pytest.raises(ZeroDivisionError):
            with ops.deterministic():
                assert ops.is_deterministic()
                1 / 0
        assert not ops.is_deterministic()
        ops.set_deterministic(True)
        with ops.deterministic(False):
            assert not ops.is_deterministic()
        assert ops.is_deterministic()
        # PyTorch's global flag is not consulted in either direction
        ops.set_deterministic(False)
        prev = torch.are_deterministic_algorithms_enabled()
        try:
            torch.use_deterministic_algorithms(True)
            assert not ops.is_deterministic()
        finally:
            torch.use_deterministic_algorithms(prev)
    finally:
        ops.set_deterministic(start)
    assert set(ops.ORDERED_KINDS).isdisjoint(ops.ATOMIC_KINDS) and len(ops.ORDERED_KINDS) == len(ops.ATOMIC_KINDS) == 7
    assert all(k.endswith("_ordered") for k in ops.ORDERED_KINDS)


@pytest.mark.parametrize("value,expected", [(None, False), ("1", True), ("0", False), ("", False), ("true", False)])
def test_environment_variable_is_read_once_at_import(value, expected):
    env = {k: v for k, v in os.environ.items() if k != "UCLSTM_DETERMINISTIC"}
    if value is not None:
        env["UCLSTM_DETERMINISTIC"] = value
    code = ("import os, sys; sys.path.insert(0, %r); import unet_convlstm_amd as U; a = U.is_deterministic(); "
            "os.environ['UCLSTM_DETERMINISTIC'] = '0' if a else '1'; print(int(a), int(U.is_deterministic()))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(int(expected))] * 2, out
