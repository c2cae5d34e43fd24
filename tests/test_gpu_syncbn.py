"""SyncBatchNorm through the whole training step: TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True) on blobs at 32 x 32,
T = 3 (the model of the two-rank FlatDDP test; it reaches the plain, the pool-fused and the head-fused BatchNorm stage).

(a) with the switch on the launch log holds the four new kernels for all three variants and two collectives per stage; with it
    off the log is what it was;
(b) one rank over gloo, deterministic mode: a train_step with the switch on leaves the bits of one with it off (loss, gradient,
    parameters after an lr = 1e-3 step, every running statistic), in bf16 and fp16 compute;
(c) two ranks on the one GPU over gloo, FlatDDP(sync_bn=True), lr = 0, unmasked loss: rank r gets sequences [2r, 2r + 2) of one
    B = 4 batch whose halves come from different blob seeds; compared with the single-process B = 4 step from rank 0's broadcast
    parameters;
(d) two ranks with B = 2 and B = 1 raise UclstmError in both processes, and neither hangs.

The bound on e_sync (rel-L2 of the synced two-rank gradient against the B = 4 gradient) is measured in the same run on code that
does not know the switch:
  e_perm  = rel-L2 between the B = 4 gradient and the same step with the batch order reversed: identical mathematics, another
            summation order (and the bf16 roundings that follow from last-bit differences in scale and shift) -- the only way a
            correct synced run may differ;
  e_local = rel-L2 between the unsynced two-rank averaged gradient and the B = 4 gradient: what the feature removes.
Required: e_local >= 1e-2 (a condition on the input), e_sync <= e_local / 100, e_sync <= max(8 * e_perm, 1e-5).  (8: the split
reorders sums in three places -- statistics, BatchNorm backward sums, weight-gradient accumulation across ranks -- and e_perm is
one sample of a noisy quantity; 1e-5 is the bound of the single-rank FlatDDP test for "same mathematics, other f32 order".)

Running statistics against the single process: within T * RTOL, RTOL = 2^-21 of the statistics test at the C ABI (T momentum steps
in order).  running_var is a sum of positive terms and is compared element by element relative to itself; running_mean has no
sign structure in a trained-from-random model (a channel's mean may be arbitrarily close to 0 while its terms are not), so its
error is taken relative to |running_mean| + sqrt(running_var), the magnitude of the terms its sums are made of.

Every child process gets init_process_group(timeout = 60 s); the parent joins with a timeout, terminates what is still alive and
fails -- nothing is retried.
"""
import datetime
import os

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import unet_convlstm_amd as U
    from unet_convlstm_amd import ops

DEV = "cuda"
T, HW = 3, 32
RTOL = 2.0 ** -21
NEW_KERNELS = ("bn_stats_partial", "bn_stats_from_sums", "bn_bwd_sums_stage", "bn_bwd_sums_finish")


def make_model(seed=77):
    torch.manual_seed(seed)
    return U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).to(DEV).train()


def make_batch():
    """One B = 4 batch: sequences 0-1 from blob seed 5, sequences 2-3 from blob seed 6 (host tensors)."""
    a = U.SyntheticSequences(2, T, HW, HW, seed=5, kind="blobs", device="cpu")
    b = U.SyntheticSequences(2, T, HW, HW, seed=6, kind="blobs", device="cpu")
    return torch.cat((a.x, b.x)), torch.cat((a.y, b.y))


@pytest.fixture
def gloo_one_rank():
    """A one-rank gloo process group in this process (destroyed afterwards if it was created here)."""
    import torch.distributed as dist
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{30500 + os.getpid() % 1500}",
                                timeout=datetime.timedelta(seconds=60))
    group = dist.new_group(ranks=[dist.get_rank()], backend="gloo", timeout=datetime.timedelta(seconds=60))
    try:
        yield group
    finally:
        U.set_sync_batchnorm(None)
        if created:
            dist.destroy_process_group()
        else:
            dist.destroy_process_group(group)


def logged_step(group, deterministic=False, dtype=torch.bfloat16):
    """One train_step from seed 77 on the first two sequences of the batch, with SyncBatchNorm over ``group`` (None: off)."""
    x, y = make_batch()
    x, y = x[:2].to(DEV), y[:2].to(DEV)
    fp16 = dtype == torch.float16
    with ops.deterministic(deterministic), ops.compute_dtype(dtype):
        model = make_model()
        opt = U.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.0, max_grad_norm=None, **(dict(loss_scale=2.0 ** 14) if fp16 else {}))
        ops.LAUNCH_LOG = []
        try:
            if group is None:
                loss, _ = U.train_step(model, opt, x, y, None, False, None, clip_norm=None)
            else:
                with U.sync_batchnorm(group):
                    loss, _ = U.train_step(model, opt, x, y, None, False, None, clip_norm=None)
            torch.cuda.synchronize()
            log = list(ops.LAUNCH_LOG)
        finally:
            ops.LAUNCH_LOG = None
    out = dict(loss=loss.cpu(), flat_g=opt.flat.flat_g.cpu(), flat_p=opt.flat.flat_p.cpu())
    out.update({"buffer " + k: b.detach().cpu() for k, b in model.named_buffers()})
    return out, log


def test_launch_log_holds_the_new_kernels_for_every_variant(gloo_one_rank):
    off, log_off = logged_step(None)
    on, log_on = logged_step(gloo_one_rank)
    assert not [e for e in log_off if e[0] in ("syncbn", "collective")], "switch off: nothing of SyncBatchNorm may be launched"
    assert [e for e in log_on if e[0] not in ("syncbn", "collective")] == log_off, "the switch changed launches that are not its own"
    for variant in ("plain", "pool", "head"):
        for kernel in NEW_KERNELS:
            assert ("syncbn", kernel, variant) in log_on, f"{kernel} not launched for the {variant} stage"
    stages = sum(1 for e in log_on if e[:2] == ("syncbn", "bn_stats_partial"))
    coll = [e for e in log_on if e[0] == "collective"]
    n_bn = sum(1 for m in U.TemporalUNetDualView(1, 1, base_ch=8, use_skip_lstm=True).modules() if isinstance(m, torch.nn.BatchNorm2d))
    print(f"[parity] SyncBatchNorm launch log: {stages} BatchNorm stages ({n_bn} BatchNorm2d modules), {len(coll)} collectives, "
          f"{sum(e[2] for e in coll)} payload bytes per step, largest {max(e[2] for e in coll)} bytes")
    assert stages == n_bn and len(coll) == 2 * stages
    assert sum(1 for e in coll if e[1] == "bn_stats") == stages and sum(1 for e in coll if e[1] == "bn_bwd_sums") == stages
    cp_max = max(ops.cpad(m.num_features) for m in make_model().modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert all(e[2] <= T * cp_max * 2 * 8 for e in coll)
    assert bool(torch.isfinite(on["loss"])) and float(on["flat_g"].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_one_rank_deterministic_step_keeps_the_bits(gloo_one_rank, dtype):
    off, _ = logged_step(None, deterministic=True, dtype=dtype)
    on, log = logged_step(gloo_one_rank, deterministic=True, dtype=dtype)
    assert any(e[0] == "collective" for e in log), "the synced path did not run"
    assert bool(torch.isfinite(off["loss"])) and float(off["flat_g"].abs().max()) > 0
    stats = [k for k in off if k.startswith("buffer ") and ("running_mean" in k or "running_var" in k)]
    assert len(stats) >= 2 * 18
    for key in off:
        same = torch.equal(off[key], on[key])
        if not same:
            print(f"[parity] one rank, switch on vs off: {key} differs, rel-L2 {rel_l2(on[key].double(), off[key].double()):.3e}")
        assert same, f"{key}: SyncBatchNorm over one rank changed the bits"
    print(f"[parity] one rank over gloo, deterministic, {dtype}: loss, gradient, parameters after the step and {len(stats)} running "
          "statistics bit-identical with the switch on and off")


# ---------------------------------------------------------------------------------------------
# two ranks on one GPU
# ---------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out_dir, sizes):
    """``sizes``: sequences per rank.  Equal sizes: the unsynced step, then the synced step from the same state; everything
    goes to rank<r>.pt.  Unequal sizes: the synced step must raise UclstmError, whose text is saved."""
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}",
                            timeout=datetime.timedelta(seconds=60))
    out = {}
    try:
        x, y = make_batch()
        lo = sum(sizes[:rank])
        x, y = x[lo:lo + sizes[rank]].to(dev), y[lo:lo + sizes[rank]].to(dev)
        model = make_model(77 + rank)                      # different initialisation per rank: the broadcast fixes it
        opt = U.FusedAdamW(model.parameters(), lr=0.0, weight_decay=0.0, max_grad_norm=None)
        ddp = U.FlatDDP(model, opt.flat, bucket_mb=0.05)
        buffers0 = {k: b.detach().clone() for k, b in model.named_buffers()}
        out["p"] = opt.flat.flat_p.cpu().clone()
        if len(set(sizes)) == 1:
            loss, _ = U.train_step(model, opt, x, y, None, False, ddp, clip_norm=None)
            torch.cuda.synchronize()
            out["g_local"], out["loss_local"] = opt.flat.flat_g.cpu().clone(), float(loss)
        ddp.remove_hooks()
        with torch.no_grad():
            for k, b in model.named_buffers():
                b.copy_(buffers0[k])
        ddp = U.FlatDDP(model, opt.flat, bucket_mb=0.05, sync_bn=True, broadcast=False)
        try:
            loss, _ = U.train_step(model, opt, x, y, None, False, ddp, clip_norm=None)
            torch.cuda.synchronize()
            out["g_sync"], out["loss_sync"] = opt.flat.flat_g.cpu().clone(), float(loss)
            out["buffers"] = {k: b.detach().cpu().clone() for k, b in model.named_buffers()}
            out["switch_after"] = U.get_sync_batchnorm() is None
        except U.UclstmError as e:
            out["uclstm_error"] = str(e)
            torch.cuda.synchronize()
    except Exception as e:                  # reported, not raised: the parent reads both ranks' files
        out["error"] = repr(e)
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def run_ranks(tmp_path, sizes):
    import torch.multiprocessing as mp
    port = 32100 + (os.getpid() % 1500)
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_worker, args=(r, len(sizes), port, str(tmp_path), sizes)) for r in range(len(sizes))]
    for p in procs:
        p.start()
    hung = False
    for p in procs:
        p.join(timeout=150)
        if p.is_alive():
            hung = True
    if hung:
        for p in procs:
            if p.is_alive():
                p.terminate()
        pytest.fail("a rank process did not finish in time")
    for p in procs:
        assert p.exitcode == 0, f"rank process exited with {p.exitcode}"
    res = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(len(sizes))]
    for r in res:
        assert "error" not in r, r.get("error")
    return res


def single_process_step(params, x, y):
    model = make_model()
    opt = U.FusedAdamW(model.parameters(), lr=0.0, weight_decay=0.0, max_grad_norm=None)
    opt.flat.flat_p.copy_(params.to(DEV))
    loss, _ = U.train_step(model, opt, x.to(DEV), y.to(DEV), None, False, None, clip_norm=None)
    torch.cuda.synchronize()
    return float(loss), opt.flat.flat_g.cpu().clone(), {k: b.detach().cpu().clone() for k, b in model.named_buffers()}


def test_two_ranks_reproduce_the_single_process_step_at_the_global_batch(tmp_path):
    r0, r1 = run_ranks(tmp_path, [2, 2])
    assert "uclstm_error" not in r0 and "uclstm_error" not in r1, (r0.get("uclstm_error"), r1.get("uclstm_error"))
    assert r0["switch_after"] and r1["switch_after"], "train_step left the switch on"
    assert torch.equal(r0["p"], r1["p"])
    # both ranks hold the same statistics and gradients
    assert torch.equal(r0["g_sync"], r1["g_sync"]) and float(r0["g_sync"].abs().max()) > 0
    for k in r0["buffers"]:
        assert torch.equal(r0["buffers"][k], r1["buffers"][k]), f"{k} differs between the ranks"
    x, y = make_batch()
    loss4, g4, buf4 = single_process_step(r0["p"], x, y)
    _, g4r, _ = single_process_step(r0["p"], x.flip(0), y.flip(0))
    e_perm = rel_l2(g4r, g4)
    e_local = rel_l2(r0["g_local"], g4)
    e_sync = rel_l2(r0["g_sync"], g4)
    loss2 = 0.5 * (r0["loss_sync"] + r1["loss_sync"])
    print(f"[parity] SyncBatchNorm 2 ranks vs single process B = 4: e_sync {e_sync:.3e}")
    print(f"[parity] single process B = 4, batch order reversed: e_perm {e_perm:.3e}")
    print(f"[parity] unsynced 2 ranks vs single process B = 4: e_local {e_local:.3e}")
    print(f"[parity] loss: mean of the two ranks {loss2:.9g}, single process {loss4:.9g}, relative difference "
          f"{abs(loss2 - loss4) / abs(loss4):.3e}; unsynced {0.5 * (r0['loss_local'] + r1['loss_local']):.9g}")
    worst_m = worst_v = 0.0
    for k, ref in buf4.items():
        got = r0["buffers"][k]
        if k.endswith("num_batches_tracked"):
            assert torch.equal(got, ref) and int(ref) == T, k
        elif k.endswith("running_var"):
            worst_v = max(worst_v, float(((got.double() - ref.double()).abs() / ref.double().abs()).max()))
        elif k.endswith("running_mean"):
            scale = ref.double().abs() + buf4[k.replace("running_mean", "running_var")].double().sqrt()
            worst_m = max(worst_m, float(((got.double() - ref.double()).abs() / scale).max()))
    print(f"[parity] running statistics vs single process: running_mean {worst_m:.3e}, running_var {worst_v:.3e} (<= {T * RTOL:.3e})")
    assert e_local >= 1e-2, f"the halves of the batch are too alike for this test: e_local {e_local:.3e}"
    assert abs(loss2 - loss4) <= 1e-6 * abs(loss4)
    assert worst_m <= T * RTOL and worst_v <= T * RTOL
    assert e_sync <= e_local / 100
    assert e_sync <= max(8 * e_perm, 1e-5)


def test_unequal_local_batches_raise_on_both_ranks(tmp_path):
    r0, r1 = run_ranks(tmp_path, [2, 1])
    for rank, r in enumerate((r0, r1)):
        assert "uclstm_error" in r, f"rank {rank} did not raise"
        assert "rank 0: (6, " in r["uclstm_error"] and "rank 1: (3, " in r["uclstm_error"], r["uclstm_error"]      # images = B * T
