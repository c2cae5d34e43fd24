"""The 4-wave / 128 x 128-per-wave form of the 256 x 256 weight-gradient kernel (igemm_wgrad_p3w_kernel, the default for
C_out >= 256) against the 8-wave form it replaces (igemm_wgrad_p3_kernel, UCLSTM_P3_WAVES=8) and against F.conv2d.

Both kernels issue the same MFMA instruction in the same k order for every output element, so at equal pixel-range splits
their slabs must agree BIT FOR BIT: any difference is a bug (a staging race, a wrong tile map), not rounding.  The switch is
read once per process, so each arm runs in a fresh child process that writes its slabs to a temporary .npz; the children run
one after the other.  The splits are set explicitly in the descriptor, so a change of the split planner cannot hide here.
Float atomics reorder, so atomic mode is compared at the rel-L2 bound of test_conv3x3_wgrad (2e-6) instead.
"""
import ctypes
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2 = 2e-6          # test_conv3x3_wgrad: f32 accumulation of 16-bit products

# (n_img, C0, C1, C_out, H, W): the six C_out >= 256 cases of test_conv3x3_wgrad ...
BASE_CASES = [
    (4, 64, 0, 256, 4, 4),          # one K-tile (64 pixels)
    (8, 256, 0, 256, 4, 4),         # two K-tiles
    (1, 136, 0, 320, 32, 32),       # partial second row tile, padded channels
    (2, 64, 64, 256, 16, 16),       # two sources
    (2, 64, 0, 512, 64, 64),        # long pixel range, W >= 64
    (6, 72, 200, 264, 8, 8),        # two sources, both padded
]
# ... and one per benchmark family at reduced pixel count: the ConvLSTM gate gradient (two sources, N = 4 * Hd = 1024) and a
# two-source UNet convolution with N = 1024 whose packed K axis (9 * 384 = 3456 columns) ends in a partial 256-column tile
FAMILY_CASES = [
    (4, 256, 256, 1024, 16, 16),
    (20, 192, 192, 1024, 4, 4),
]

# Runs in the child (and, for the reproducibility test, in this process): same seeds -> same operands in every process.
HELPERS = textwrap.dedent("""
    import ctypes
    import torch

    def cpad(c):
        return (c + 7) // 8 * 8

    def make_operands(case, dtype):
        N, C0, C1, Co, H, W = case
        g = torch.Generator().manual_seed(1000 + 7 * Co + C0 + C1 + H)
        x0 = torch.randn(N, C0, H, W, generator=g).to(dtype).float()
        x1 = torch.randn(N, C1, H, W, generator=g).to(dtype).float() if C1 else None
        dy = torch.randn(N, Co, H, W, generator=g).to(dtype).float()
        return x0, x1, dy

    def to_nhwc(x, dtype):
        N, C, H, W = x.shape
        t = torch.zeros(N, H, W, cpad(C))
        t[..., :C] = x.permute(0, 2, 3, 1)
        return t.to(dtype).cuda().contiguous()

    def run_wgrad(case, dtype, splits, atomic):
        '''-> (slabs [splits, N, Ktot] or the atomically accumulated panel [1, N, Ktot], unpacked gradient, kernel shape)'''
        import unet_convlstm_amd as U
        from unet_convlstm_amd import ops
        N, C0, C1, Co, H, W = case
        x0, x1, dy = make_operands(case, dtype)
        srcs = [ops.SrcView(to_nhwc(x0, dtype))] + ([ops.SrcView(to_nhwc(x1, dtype))] if C1 else [])
        cv = [C0] + ([C1] if C1 else [])
        pd = ops.conv_pack_desc(Co, C0 + C1, cv, [cpad(c) for c in cv])
        dyn = to_nhwc(dy, dtype)
        wd = U._lib.WgradDesc()
        wd.n_img, wd.H, wd.W, wd.ktap, wd.scale, wd.pad, wd.nsrc = N, H, W, 3, 1, 1, len(srcs)
        for i, sv in enumerate(srcs):
            sv.fill(wd.src[i])
        wd.N, wd.Ktot, wd.nseg = pd.N, pd.Ktot, 1
        ops._fill_seg(wd.seg[0], dyn, 0, cpad(Co), 0, 1, 0, 0)
        wd.splits, wd.accumulate, wd.slab = splits, 1, (0 if atomic else pd.N * pd.Ktot)
        shape = int(U._lib.lib.uclstm_igemm_wgrad_shape(ctypes.byref(wd)))
        used = int(U._lib.lib.uclstm_igemm_wgrad_splits(ctypes.byref(wd)))      # ranges that own pixels (<= splits)
        assert 1 <= used <= splits, (used, splits)
        if atomic:
            dwp = torch.zeros(1, pd.N, pd.Ktot, device="cuda")
        else:
            dwp = torch.full((used, pd.N, pd.Ktot), float("nan"), device="cuda")
            wd.splits = used
        wd.dwp = dwp.data_ptr()
        U._lib.check(ops._k(dyn).uclstm_igemm_wgrad(ctypes.byref(wd), ops._stream()), "igemm_wgrad")
        torch.cuda.synchronize()
        got = ops.unpack_wgrad(pd, dwp if not atomic else dwp[0], torch.zeros(Co, C0 + C1, 3, 3, device="cuda"))
        return dwp, got, shape
""")

CHILD = HELPERS + textwrap.dedent("""
    import json, sys
    import numpy as np
    sys.path.insert(0, sys.argv[1])
    jobs = json.loads(sys.argv[2])
    dtype = torch.float16 if sys.argv[3] == "f16" else torch.bfloat16
    out = {}
    for i, (case, splits, atomic) in enumerate(jobs):
        dwp, got, shape = run_wgrad(tuple(case), dtype, splits, bool(atomic))
        assert shape == 3, (case, shape)
        out["dwp%d" % i] = dwp.cpu().numpy()
        out["got%d" % i] = got.cpu().numpy()
    np.savez(sys.argv[4], **out)
""")

exec(HELPERS)      # make_operands / run_wgrad for this process  # noqa: S102


def _jobs():
    jobs = [(c, s, 0) for c in BASE_CASES for s in (1, 3)]
    jobs += [(c, s, a) for c in FAMILY_CASES for s in (1, 3) for a in (0, 1)]
    return jobs


def _run_child(tmp_path, tag, dt, env_extra):
    f = str(tmp_path / f"{tag}_{dt}.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("UCLSTM_P3_WAVES", "UCLSTM_P3_LEAD")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT_DIR, json.dumps(_jobs()), dt, f], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"{tag} child failed ({r.returncode}): {r.stderr[-2000:]}"
    return np.load(f)


def _reference(case, dtype):
    x0, x1, dy = make_operands(case, dtype)      # noqa: F821
    xin = x0 if x1 is None else torch.cat((x0, x1), 1)
    w = torch.zeros(case[3], xin.shape[1], 3, 3, requires_grad=True)
    (F.conv2d(xin, w, None, padding=1) * dy).sum().backward()
    return w.grad


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_wide_kernel_is_bit_identical_to_the_8_wave_kernel_and_matches_conv2d(tmp_path, dt):
    """Slab mode: every slab of the 4-wave kernel equals the 8-wave kernel's bit for bit (deep and shallow DMA ring).  Atomic
    mode: rel-L2 <= 2e-6 between the two.  Every result of the 4-wave kernel: rel-L2 <= 2e-6 against the F.conv2d f32 gradient."""
    dtype = torch.float16 if dt == "f16" else torch.bfloat16
    old = _run_child(tmp_path, "waves8", dt, {"UCLSTM_P3_WAVES": "8"})
    new = _run_child(tmp_path, "waves4", dt, {})
    shallow = _run_child(tmp_path, "waves4_lead8", dt, {"UCLSTM_P3_LEAD": "6"})
    refs = {}
    bad = []
    for i, (case, splits, atomic) in enumerate(_jobs()):
        a, b, c = old[f"dwp{i}"], new[f"dwp{i}"], shallow[f"dwp{i}"]
        assert a.shape == b.shape == c.shape and np.isfinite(b).all() and np.isfinite(c).all(), (case, splits, atomic)
        what = f"{dt} case {case} splits {splits} {'atomic' if atomic else 'slabs'}"
        if atomic:
            for arm, v in (("deep", b), ("shallow", c)):
                e = rel_l2(torch.from_numpy(v), torch.from_numpy(a))
                print(f"[parity] {what} 4-wave ({arm}) vs 8-wave: rel-L2 {e:.3e} (tol {L2})")
                if not e <= L2:
                    bad.append(f"{what}: {arm} ring vs 8-wave rel-L2 {e:.3e}")
        else:
            for arm, v in (("deep", b), ("shallow", c)):
                if not np.array_equal(a.view(np.uint32), v.view(np.uint32)):
                    n = int((a.view(np.uint32) != v.view(np.uint32)).sum())
                    bad.append(f"{what}: {arm} ring differs from the 8-wave kernel in {n} of {a.size} elements")
        if case not in refs:
            refs[case] = _reference(case, dtype)
        for arm, res in (("deep", new), ("shallow", shallow)):
            e = rel_l2(torch.from_numpy(res[f"got{i}"]), refs[case])
            print(f"[parity] {what} 4-wave ({arm}) vs conv2d: rel-L2 {e:.3e} (tol {L2})")
            if not e <= L2:
                bad.append(f"{what}: {arm} ring vs conv2d rel-L2 {e:.3e}")
    assert not bad, "\n".join(bad)


def test_wide_kernel_is_reproducible_run_to_run():
    """A staging race shows as values that change between runs: the largest cases twenty times in one process, slab mode,
    every result bit-equal to the first."""
    for case, splits in ((FAMILY_CASES[0], 3), (BASE_CASES[4], 3), (FAMILY_CASES[1], 1)):
        first = None
        for run in range(20):
            dwp, _, shape = run_wgrad(case, torch.bfloat16, splits, False)      # noqa: F821
            assert shape == 3
            v = dwp.cpu().numpy().view(np.uint32)
            if first is None:
                first = v
                assert np.isfinite(dwp.cpu().numpy()).all()
            else:
                assert np.array_equal(first, v), f"case {case}: run {run} differs from run 0 in {int((first != v).sum())} elements"
