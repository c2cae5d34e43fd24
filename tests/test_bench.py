"""bench.py: what a plain run prints and what --dump-outputs writes (the launch contract is in test_cabi_and_host.py)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float32_and_a_fixed_sample_of_a_large_array(tmp_path):
    b = _bench_module()
    n = b.DUMP_MAX_VALUES + 4096
    big = torch.arange(n, dtype=torch.float64).reshape(-1, 8)          # value = flat index (exact in float32 below 2^24)
    small = torch.linspace(-1, 1, 60, dtype=torch.bfloat16).reshape(3, 4, 5)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), big=big, small=small, loss=torch.tensor(1.25))
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("big", "small", "loss")}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["small"].shape == (3, 4, 5) and np.array_equal(got["small"], small.float().numpy())
    assert got["loss"].shape == () and float(got["loss"]) == 1.25
    s = got["big"]
    assert s.shape == (b.DUMP_MAX_VALUES,) and np.all(np.diff(s) >= 0) and s[0] >= 0 and s[-1] < n
    assert s[-1] - s[0] > 0.99 * n                                      # spread over the whole array, not one block of it
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))      # the same indices in every run
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) < 64e6


@pytest.mark.gpu
def test_plain_run_times_the_given_steps_and_dumps_the_last_one(tmp_path):
    """A plain run prints the contract fields for exactly --steps timed steps and none of the --full parts; --dump-outputs
    writes the loss and the prediction of the last timed step, and a second run with the same arguments writes the same
    values to rounding (the step's float atomics sum in a different order)."""
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "4", "--warmup", "2", "--base-ch", "8", "--batch", "2",
                            "--seq", "3", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = outs[0]
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(out)
    assert not {"roofline", "secondary", "side_stream", "cpu_baseline"} & set(out)
    assert out["steps"] == 4 and "headline: timed 4 steps" in r.stderr
    assert out["value"] * out["ms_per_step"] / 1e3 == pytest.approx(2 * 3, rel=1e-2)      # frames of ONE step
    (la, ya), (lb, yb) = ((np.load(tmp_path / d / "loss.npy"), np.load(tmp_path / d / "y_pred.npy")) for d in ("a", "b"))
    assert la.dtype == np.float32 and ya.dtype == np.float32 and ya.shape == (2, 3, 1, 64, 64) and np.isfinite(ya).all()
    assert float(la) == pytest.approx(out["final_loss"], abs=1e-5)
    ya, yb = ya.astype(np.float64), yb.astype(np.float64)
    assert abs(float(la) - float(lb)) <= 1e-4 * abs(float(lb)) and np.linalg.norm(ya - yb) <= 1e-3 * np.linalg.norm(yb)
