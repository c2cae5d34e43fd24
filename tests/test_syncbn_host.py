"""SyncBatchNorm, the parts that need no GPU: the four additive entry points in the header and the library (ABI version
unchanged), the switch and its refusals, and FlatDDP(sync_bn=True) in the two-rank gloo CPU setup of test_cabi_and_host.py (as
far as that setup goes without device tensors: construction, the flag, the gradient exchange and the switch's state around it)."""
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib, ops
from unet_convlstm_amd.ddp import FlatDDP
from unet_convlstm_amd.optim import FlatParams

NEW = ["uclstm_bn_stats_partial", "uclstm_bn_stats_from_sums", "uclstm_bn_bwd_sums_stage", "uclstm_bn_bwd_sums_finish"]


def test_new_entry_points_are_declared_exported_and_additive():
    syms = _lib.header_symbols()
    for name in NEW:
        assert name in syms, f"{name} is not declared in include/uclstm.h"
        assert hasattr(_lib.lib, name), f"{name} is not exported by the library"
        assert name in _lib._PROTOS and name not in _lib.F16_TWINS
        assert not hasattr(_lib.lib, name + "_f16"), f"{name} works on f32 / f64 statistics only and has no fp16 twin"
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert re.search(r"^#define UCLSTM_ABI_VERSION 16$", text, re.M)
    assert _lib.ABI_VERSION == 16 and _lib.lib.uclstm_abi_version() == 16


def test_bad_arguments_are_refused_before_any_launch():
    """Null pointers, empty shapes and an inv_world outside (0, 1] return UCLSTM_E_BADARG (-1); nothing is launched, so this
    runs without a device."""
    lib, one = _lib.lib, 16          # a non-null, 16-byte aligned address that is never dereferenced: every call fails its checks
    assert lib.uclstm_bn_stats_partial(None, 1, 1, 8, one, None) == -1
    assert lib.uclstm_bn_stats_partial(one, 1, 1, 8, None, None) == -1
    assert lib.uclstm_bn_stats_partial(one, 0, 1, 8, one, None) == -1
    assert lib.uclstm_bn_stats_partial(one, 1, 1, 8, 24, None) == -1            # sums64 not 16-byte aligned
    assert lib.uclstm_bn_stats_from_sums(one, 0, one, 1, 1, 8, 8, one, one, 1e-5, one, one, one, one, None) == -1     # count 0
    assert lib.uclstm_bn_stats_from_sums(one, 4, one, 1, 1, 8, 9, one, one, 1e-5, one, one, one, one, None) == -1     # C > Cp
    assert lib.uclstm_bn_stats_from_sums(None, 4, one, 1, 1, 8, 8, one, one, 1e-5, one, one, one, one, None) == -1
    assert lib.uclstm_bn_bwd_sums_stage(one, one, 0, None) == -1
    assert lib.uclstm_bn_bwd_sums_stage(None, one, 16, None) == -1
    assert lib.uclstm_bn_bwd_sums_finish(one, 0.0, one, 16, None) == -1
    assert lib.uclstm_bn_bwd_sums_finish(one, 2.0, one, 16, None) == -1
    assert lib.uclstm_bn_bwd_sums_finish(one, 0.5, None, 16, None) == -1


def test_switch_is_off_by_default_and_needs_a_process_group():
    assert not dist.is_initialized()
    assert U.get_sync_batchnorm() is None
    with pytest.raises(U.UclstmError, match="not initialised"):
        U.set_sync_batchnorm(True)
    with pytest.raises(U.UclstmError, match="not initialised"):
        with U.sync_batchnorm():
            pass
    assert U.get_sync_batchnorm() is None
    U.set_sync_batchnorm(None)                # turning it off never needs one
    U.set_sync_batchnorm(False)
    assert U.get_sync_batchnorm() is None
    assert ops.sync_batchnorm is U.sync_batchnorm and ops.set_sync_batchnorm is U.set_sync_batchnorm


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import datetime
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    out = {}
    try:
        torch.manual_seed(100 + rank)
        net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.ReLU(), torch.nn.Linear(16, 2))
        fp = FlatParams(net.parameters())
        plain = FlatDDP(net, fp)
        out["default"] = plain.sync_bn
        plain.remove_hooks()
        ddp = FlatDDP(net, fp, sync_bn=True)
        out["flag"] = ddp.sync_bn
        # the switch: on with the default group, on with an explicit group, nested, restored on exit and on an exception
        out["off0"] = U.get_sync_batchnorm() is None
        with U.sync_batchnorm():
            out["on_default"] = U.get_sync_batchnorm() is True
            with U.sync_batchnorm(dist.group.WORLD):
                out["on_group"] = U.get_sync_batchnorm() is dist.group.WORLD
            out["restored_inner"] = U.get_sync_batchnorm() is True
        out["off1"] = U.get_sync_batchnorm() is None
        try:
            with U.sync_batchnorm():
                raise KeyError("x")
        except KeyError:
            pass
        out["off2"] = U.get_sync_batchnorm() is None
        U.set_sync_batchnorm(True)
        out["set_true"] = U.get_sync_batchnorm() is True
        U.set_sync_batchnorm(None)
        out["set_none"] = U.get_sync_batchnorm() is None
        # the equal-work check: one host-side collective per distinct shape, then cached; unequal shapes raise on every rank
        w = ops._sync_bn_check_equal(None, 6, 32, 32, 3)
        out["world"] = w
        out["cached"] = (None, 6, 32, 32, 3) in ops._SYNC_BN_CHECKED
        try:
            ops._sync_bn_check_equal(None, 7 - 3 * rank, 32, 32, 3)      # a shape neither rank has checked before
            out["unequal"] = "no error"
        except U.UclstmError as e:
            out["unequal"] = str(e)
        # train_step with a CPU model: the flag is accepted, the switch stays off (no device tensors, nothing to synchronise),
        # and the gradients are exchanged as without it
        torch.manual_seed(7 + rank)
        x = torch.randn(8, 6)
        fp.zero_grad()
        ddp.reset()
        net(x).pow(2).mean().backward()
        ddp.finalize()
        out["g"] = fp.flat_g.numpy().copy()
        out["off3"] = U.get_sync_batchnorm() is None
    except Exception as e:          # reported, not raised: the parent must see both ranks' results
        out["error"] = repr(e)
    q.put((rank, out))
    dist.destroy_process_group()


def test_flat_ddp_accepts_sync_bn_in_the_two_rank_gloo_setup():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=120) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
                pytest.fail("a rank process did not finish")
    for rank in (0, 1):
        r = res[rank]
        assert "error" not in r, r.get("error")
        assert r["default"] is False and r["flag"] is True
        for k in ("off0", "on_default", "on_group", "restored_inner", "off1", "off2", "set_true", "set_none", "cached", "off3"):
            assert r[k] is True, (rank, k)
        assert r["world"] == 2
        assert "rank 0: (7, 32, 32, 3)" in r["unequal"] and "rank 1: (4, 32, 32, 3)" in r["unequal"], r["unequal"]
    assert (res[0]["g"] == res[1]["g"]).all() and float(abs(res[0]["g"]).max()) > 0
