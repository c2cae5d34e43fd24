"""CPU-only tests of the device-resident loader: the C ABI of uclstm_dataset_gather_transform (symbols, argument contract --
nothing is launched) and the epoch-row helper of DeviceSequenceLoader against a CPU DataLoader over the same sampler."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, RandomSampler, Subset, random_split

import unet_convlstm_amd as U
from unet_convlstm_amd import _lib as L

SYM = "uclstm_dataset_gather_transform"


# ---------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------
def test_gather_transform_is_in_the_header_the_binding_and_the_library():
    hdr = open(L.HEADER_PATH).read()
    raw = C.CDLL(L.LIB_PATH)
    assert re.search(r"\b%s\s*\(" % SYM, hdr)
    assert SYM in L._PROTOS and SYM in L.header_symbols() and hasattr(raw, SYM)
    assert L.lib.uclstm_abi_version() == L.ABI_VERSION == 16            # additive change
    assert int(re.search(r"#define UCLSTM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 16
    assert len(L.F16_TWINS) == 29 and SYM not in L.F16_TWINS and not hasattr(raw, SYM + "_f16")
    # the binding has one ctypes type per declared parameter
    params = re.search(r"\b%s\s*\(([^)]*)\)" % SYM, hdr).group(1)
    assert len([a for a in params.split(",") if a.strip()]) == len(L._PROTOS[SYM]) == 20
    # the old entry point is still there, unchanged in arity
    assert len(L._PROTOS["uclstm_dataset_transform"]) == 16 and hasattr(raw, "uclstm_dataset_transform")


def _args(**over):
    """Arguments that pass validation (the pointers are garbage, 16-byte aligned: a call that accepted them would launch)."""
    a = dict(x_all=0x1000, y_all=0x2000, idx=0x3000, n_seq=8, n_out=4, T=3, C=2, HW=64, x=0x4000, y=0x5000, mask=0x6000,
             transform=1, norm_const=30.0, min_vel=-7.5, max_vel=8.5, clip=1, y_scale=2.0, trans_min=-2.0, trans_max=2.2)
    a.update(over)
    return [a[k] for k in ("x_all", "y_all", "idx", "n_seq", "n_out", "T", "C", "HW", "x", "y", "mask", "transform", "norm_const",
                           "min_vel", "max_vel", "clip", "y_scale", "trans_min", "trans_max")] + [None]


BAD = {
    "null x_all": dict(x_all=None), "null y_all": dict(y_all=None), "null x": dict(x=None), "null y": dict(y=None),
    "null mask": dict(mask=None),
    "n_seq = 0": dict(n_seq=0), "n_seq < 0": dict(n_seq=-1), "n_out = 0": dict(n_out=0), "n_out < 0": dict(n_out=-3),
    "T = 0": dict(T=0), "T < 0": dict(T=-1), "C = 0": dict(C=0), "C < 0": dict(C=-2), "HW = 0": dict(HW=0), "HW < 0": dict(HW=-64),
    "transform 3": dict(transform=3), "transform -1": dict(transform=-1),
    "trans_max == trans_min": dict(trans_max=-2.0),
    "asinh with y_scale = 0": dict(transform=1, y_scale=0.0), "asinh with y_scale < 0": dict(transform=1, y_scale=-2.0),
    "signed_log with y_scale = 0": dict(transform=2, y_scale=0.0), "signed_log with y_scale < 0": dict(transform=2, y_scale=-1.0),
    "identity index with n_out > n_seq": dict(idx=None, n_out=9),
    "2^31 pixels": dict(n_seq=1 << 20, n_out=1 << 15, T=1 << 4, HW=1 << 12),
    "beyond 2^31 pixels": dict(n_seq=1 << 40, n_out=1 << 40, T=1 << 20, HW=1 << 20),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_gather_transform_rejects_bad_arguments_before_any_launch(name):
    # no GPU here and the pointers are garbage: anything but an early UCLSTM_E_BADARG would be a launch error (-2) or a crash
    assert L.lib.uclstm_dataset_gather_transform(*_args(**BAD[name])) == -1, name


# ---------------------------------------------------------------------------------------------
# epoch rows == DataLoader over the same sampler
# ---------------------------------------------------------------------------------------------
N, B = 10, 4


@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    rng = np.random.default_rng(5)
    X = (rng.random((N, 2, 2, 4, 4)) * 30).astype(np.float32)
    X[:, 0, 0, 0, 0] = np.arange(N)                    # the row's own number, readable from a collated batch
    Y = rng.normal(0, 3, (N, 2, 1, 4, 4)).astype(np.float32)
    path = tmp_path_factory.mktemp("loader") / "ds.npz"
    np.savez(path, X=X, Y=Y)
    return U.NPZSequenceDataset(str(path))


def _G(seed):
    return torch.Generator().manual_seed(seed)


def _rows_of(batch, ds):
    """Which dataset rows a collated host batch holds (x[:, 0, 0, 0, 0] * norm_const is the row number)."""
    return [int(round(float(v) * ds.norm_const)) for v in batch[0][:, 0, 0, 0, 0]]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("which", ["dataset", "split0", "split1", "nested"])
def test_epoch_rows_equal_the_dataloader_batches(ds, which, drop_last):
    a, b = random_split(ds, [7, 3], generator=_G(3))
    data = {"dataset": ds, "split0": a, "split1": b, "nested": Subset(a, [5, 0, 2, 6, 1])}[which]
    host = DataLoader(data, batch_size=B, sampler=RandomSampler(data, generator=_G(7)), drop_last=drop_last)
    mine = RandomSampler(data, generator=_G(7))
    seen = []
    for _ in range(3):
        want = [_rows_of(batch, ds) for batch in host]
        got = [r.tolist() for r in U.epoch_rows(data, mine, B, drop_last)]
        assert got == want and len(got) == len(host)
        assert all(r.dtype == np.int64 for r in U.epoch_rows(data, None, B, drop_last))
        seen.append(got)
    if len(data) > 3:
        assert seen[0] != seen[1] or seen[1] != seen[2]              # the sampler's state advances from epoch to epoch
    # in order without a sampler
    seq = [_rows_of(batch, ds) for batch in DataLoader(data, batch_size=B, drop_last=drop_last)]
    assert [r.tolist() for r in U.epoch_rows(data, None, B, drop_last)] == seq


def test_out_of_range_rows_raise_index_error(ds):
    for bad in ([0, N], [-1, 2]):
        with pytest.raises(IndexError):
            U.epoch_rows(ds, bad, B)
        with pytest.raises(IndexError):
            U.epoch_rows(Subset(ds, bad), None, B)
    with pytest.raises(IndexError):
        U.epoch_rows(Subset(ds, [1, 2, 3]), [0, 3], B)              # position 3 of a 3-element Subset
    with pytest.raises(IndexError):
        U.epoch_rows(Subset(Subset(ds, [1, 2, 3]), [0, 5]), None, B)


def test_a_non_dataset_raises_type_error(ds):
    for bad in ([1, 2, 3], torch.utils.data.TensorDataset(torch.zeros(4, 2)), Subset(torch.utils.data.TensorDataset(torch.zeros(4, 2)), [0])):
        with pytest.raises(TypeError):
            U.epoch_rows(bad, None, B)
        with pytest.raises(TypeError):
            U.DeviceSequenceLoader(bad, B)


def test_a_cpu_device_and_bad_options_raise_before_the_gpu_is_touched(ds):
    with pytest.raises(U.UclstmError):
        U.DeviceSequenceLoader(ds, B, device="cpu")
    with pytest.raises(ValueError):
        U.DeviceSequenceLoader(ds, 0, device="cpu")
    with pytest.raises(ValueError):
        U.DeviceSequenceLoader(ds, B, shuffle=True, sampler=[0, 1], device="cpu")


def test_distributed_sampler_shards_like_the_dataloader(ds):
    from torch.utils.data.distributed import DistributedSampler
    seen = []
    for rank in range(2):
        host = DistributedSampler(ds, num_replicas=2, rank=rank, shuffle=True, seed=3)
        mine = DistributedSampler(ds, num_replicas=2, rank=rank, shuffle=True, seed=3)
        for epoch in range(2):
            host.set_epoch(epoch)
            mine.set_epoch(epoch)                       # the caller's job, as with a DataLoader
            want = [_rows_of(batch, ds) for batch in DataLoader(ds, batch_size=B, sampler=host)]
            got = [r.tolist() for r in U.epoch_rows(ds, mine, B)]
            assert got == want
        seen += [r for b in got for r in b]
    assert sorted(seen) == list(range(N))               # the two ranks cover the dataset
