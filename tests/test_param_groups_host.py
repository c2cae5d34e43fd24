"""Parameter groups of FusedAdamW, host side (no GPU): the run-table builder and its checker, the constructor's contracts on
CPU parameters, and the C ABI of uclstm_adamw_step_groups (header, ctypes table, library, argument validation before any
launch)."""
import ctypes as C
import random
import re

import pytest
import torch

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L
from unet_convlstm_amd.optim import build_run_table, check_run_table


def test_run_table_merges_neighbours_of_one_group():
    sizes = [21, 5, 72, 1, 64, 1152]
    assert build_run_table(sizes, [0, 1, 0, 1, 1, 2]) == [(0, 21, 0), (21, 26, 1), (26, 98, 0), (98, 163, 1), (163, 1315, 2)]
    assert build_run_table(sizes, [0] * 6) == [(0, 1315, 0)]
    assert build_run_table(sizes, [3, 3, 3, 0, 0, 3]) == [(0, 98, 3), (98, 163, 0), (163, 1315, 3)]
    assert build_run_table([1], [0]) == [(0, 1, 0)]
    with pytest.raises(ValueError):
        build_run_table([4, 4], [0])
    with pytest.raises(ValueError):
        build_run_table([4, 0], [0, 1])
    with pytest.raises(ValueError):
        build_run_table([4, 4], [0, -1])


def test_run_table_seeded_sweep_is_sorted_gap_free_and_names_the_right_group():
    rng = random.Random(20240611)
    for _ in range(300):
        k = rng.randint(1, 120)
        n_groups = rng.randint(1, 6)
        sizes = [rng.choice([1, 1, 2, 7, 64, 255, 256, 257, 1000, rng.randint(1, 50000)]) for _ in range(k)]
        groups = [rng.randrange(n_groups) for _ in range(k)]
        runs = build_run_table(sizes, groups)
        n = sum(sizes)
        check_run_table(runs, n, n_groups)
        assert runs[0][0] == 0 and runs[-1][1] == n
        assert all(a[1] == b[0] and a[2] != b[2] for a, b in zip(runs, runs[1:]))          # gap-free, neighbours merged
        assert all(b < e and 0 <= g < n_groups for b, e, g in runs)
        # every tensor lies inside one run of its own group
        off, r = 0, 0
        for s, g in zip(sizes, groups):
            while runs[r][1] <= off:
                r += 1
            assert runs[r][0] <= off and off + s <= runs[r][1] and runs[r][2] == g
            off += s
        assert len(runs) <= k


def test_run_table_checker_refuses_what_the_kernel_must_not_walk():
    good = [(0, 10, 0), (10, 11, 1), (11, 40, 0)]
    check_run_table(good, 40, 2)
    for bad, n, ng in (([], 40, 2),
                       ([(0, 10, 0), (11, 40, 1)], 40, 2),                 # gap
                       ([(0, 10, 0), (9, 40, 1)], 40, 2),                  # overlap
                       ([(10, 40, 1), (0, 10, 0)], 40, 2),                 # not sorted
                       ([(1, 40, 0)], 40, 1),                              # does not begin at 0
                       ([(0, 10, 0), (10, 10, 1), (10, 40, 0)], 40, 2),    # empty run
                       (good, 41, 2),                                      # does not reach n
                       (good, 39, 2),
                       (good, 40, 1),                                      # group index out of range
                       ([(0, 40, -1)], 40, 1)):
        with pytest.raises(ValueError):
            check_run_table(bad, n, ng)


def _params(shapes):
    return [torch.nn.Parameter(torch.zeros(s)) for s in shapes]


def test_groups_on_cpu_parameters_raise_the_no_cpu_path_error():
    a, b, c = _params([(3, 2), (4,), (2, 2)])
    with pytest.raises(RuntimeError, match="needs HIP device parameters"):
        U.FusedAdamW([{"params": [a, c], "weight_decay": 1e-2}, {"params": [b], "weight_decay": 0.0, "lr": 1e-4}])
    with pytest.raises(RuntimeError, match="needs HIP device parameters"):
        U.FusedAdamW([{"params": [a, c]}, {"params": [b], "weight_decay": 0.0}], order=[a, b, c], capturable=True, loss_scale=1024.0)


def test_order_must_agree_with_the_groups():
    a, b, c = _params([(3, 2), (4,), (2, 2)])
    with pytest.raises(ValueError, match="in no parameter group"):
        U.FusedAdamW([{"params": [a]}, {"params": [b]}], order=[a, b, c])
    with pytest.raises(ValueError, match="not in `order`"):
        U.FusedAdamW([{"params": [a]}, {"params": [b, c]}], order=[a, b])
    with pytest.raises(ValueError, match="twice"):
        U.FusedAdamW([{"params": [a]}, {"params": [b]}], order=[a, b, a])
    with pytest.raises(ValueError):                                       # torch.optim.Optimizer's own check
        U.FusedAdamW([{"params": [a, b]}, {"params": [b]}])
    # a frozen parameter of `order` needs no group (fine-tuning: order=model.parameters(), groups over the trainable ones);
    # the constructor then gets as far as the device check
    c.requires_grad_(False)
    with pytest.raises(RuntimeError, match="needs HIP device parameters"):
        U.FusedAdamW([{"params": [a]}, {"params": [b]}], order=[a, b, c])


def test_header_ctypes_table_and_library_agree_on_the_groups_entry_point():
    hdr = open(L.HEADER_PATH).read()
    assert "uclstm_adamw_step_groups" in L.header_symbols() and "uclstm_adamw_step_groups" in L._PROTOS
    assert int(re.search(r"#define UCLSTM_ABI_VERSION (\d+)", hdr).group(1)) == 16 == L.ABI_VERSION == L.lib.uclstm_abi_version()
    m = re.search(r"int32_t uclstm_adamw_step_groups\(([^)]*)\)", hdr)
    assert m is not None
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(L._PROTOS["uclstm_adamw_step_groups"]) == 12
    assert "uclstm_adamw_step_groups" not in L.F16_TWINS                  # f32 only, like its neighbours


def test_groups_entry_point_validates_before_any_launch():
    buf = (C.c_float * 64)()                       # 16-byte aligned host memory: never dereferenced, every call returns first
    p = C.cast(buf, C.c_void_p)
    assert C.addressof(buf) % 16 == 0
    f = L.lib.uclstm_adamw_step_groups
    ok = [p, p, p, p, 64, p, p, 1, p, 1, None, None]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, 0), (4, -5), (6, None), (7, 0), (7, -1), (8, None), (9, 0), (9, -2),
                   (9, 1025)):
        args = list(ok)
        args[i] = bad
        assert f(*args) == -1, (i, bad)
    args = list(ok)
    args[5], args[10] = None, p                    # loss scaling needs the sum of squares
    assert f(*args) == -1
    args = list(ok)
    args[8] = C.c_void_p(C.addressof(buf) + 4)     # hyper table not 16-byte aligned
    assert f(*args) == -1
