#!/usr/bin/env python
"""Generate tests/golden/sprites.npz by running the REFERENCE's Moving-MNIST generator itself.

Run in the build container only (the reference checkout does not travel):

    python tests/golden/make_sprites_golden.py [/root/reference]

It imports the reference's ``digits/build_moving_mnist.py`` with a stub ``torchvision`` registered in ``sys.modules`` (the real
one would download MNIST): the stub's ``datasets.MNIST(...).data`` is a stand-in bank of 12 procedural 28 x 28 glyphs.  Per
case ``np.random`` is seeded and ``generate_moving_mnist`` runs; then the seed is set again and the generator's call order is
replayed to record what it drew -- per sequence and digit: ``randint(0, K)`` (the glyph), ``randint(0, S - 27, size=2)`` (x, y),
``randint(-5, 6, size=2)`` (vx, vy).

The fixture is data only (arrays: the bank, and per case the configuration, the draw table and the reference's output); no
reference source text is stored.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, ROOT)

import unet_convlstm_amd as U  # noqa: E402

# (N, T, size, digits): the defaults on the 16-byte path; a long walk; the frame equals the glyph (every non-zero velocity bounces
# every step); a width that is no multiple of 4 with heavily overlapping sprites; a single frame with one digit
CASES = [(6, 12, 64, 2), (4, 40, 64, 3), (5, 9, 28, 2), (5, 9, 31, 4), (3, 1, 64, 1)]
SEED0 = 20240


def reference_generator(bank):
    class _MNIST:
        def __init__(self, *a, **k):
            self.data = torch.from_numpy(bank)

    tv = types.ModuleType("torchvision")
    tv.datasets = types.ModuleType("torchvision.datasets")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.datasets.MNIST = _MNIST
    tv.transforms.ToTensor = lambda: None
    sys.modules.update({"torchvision": tv, "torchvision.datasets": tv.datasets, "torchvision.transforms": tv.transforms})
    spec = importlib.util.spec_from_file_location("ref_build_moving_mnist", os.path.join(REF, "digits", "build_moving_mnist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.generate_moving_mnist


def replay(seed, K, N, S, digits):
    np.random.seed(seed)
    tab = np.zeros((N, digits, 5), dtype=np.int32)
    for i in range(N):
        for d in range(digits):
            g = np.random.randint(0, K)
            x, y = np.random.randint(0, S - 28 + 1, size=2)
            vx, vy = np.random.randint(-5, 6, size=2)
            tab[i, d] = (g, x, y, vx, vy)
    return tab


def main():
    bank = U.procedural_glyphs(12, 28, seed=0)
    gen = reference_generator(bank)
    out = {"bank": bank, "cases": np.asarray(CASES, dtype=np.int32)}
    for i, (N, T, S, digits) in enumerate(CASES):
        np.random.seed(SEED0 + i)
        data = gen(seq_len=T, num_samples=N, image_size=S, num_digits=digits)
        tab = replay(SEED0 + i, len(bank), N, S, digits)
        assert data.dtype == np.float32 and data.shape == (N, T, 2, S, S)
        # the replayed table really is what the reference drew: the host mirror reproduces its output bit for bit
        assert np.array_equal(U.render_sprites_host(bank, tab, T, S, S), data), f"case {i}: the replayed draws do not reproduce the output"
        out[f"c{i}_table"], out[f"c{i}_data"] = tab, data
        print(f"case {i} {(N, T, S, digits)}: |vmap| up to {np.abs(data[:, :, 1]).max():.0f}, {100 * (data[:, :, 0] > 0).mean():.1f} % covered")
    path = os.path.join(HERE, "sprites.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
