"""Code-object check of the ring kernel's fragment pipeline (host only: `hipcc -S --cuda-device-only` needs no GPU).

`igemm_fwd_c64_kernel` runs one wave per SIMD with no barrier inside a tile, so nothing hides an LDS round trip the wave waits
for: the eight `ds_read_b128` of step s+1 have to be in flight under the MFMAs of step s, and the waits in front of a step's MFMAs
have to be counted.  tools/audit_lds_waits.py reduces the emitted tile loop to its MFMA / read / wait / barrier / DMA events; this
test asserts, on the bf16 pass, what the kernel's comment promises (the fp16 twin is audited in profiles/fwd_read_pipeline_audit.txt).
"""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("audit_lds_waits", os.path.join(ROOT, "tools", "audit_lds_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_event_string_and_exposed_reads_on_a_hand_written_listing():
    """The parser on a listing small enough to check by eye: one loop, one exposed read, one counted wait."""
    A = _tool()
    asm = "\n".join([
        "\t.type\tk,@function", "k:", "\ts_waitcnt vmcnt(0)", ".LBB0_1:", "\ts_barrier",
        "\tbuffer_load_dwordx4 v1, s[0:3], s4 offen lds", "\tds_read_b128 v[0:3], v9", "\tds_read_b128 v[4:7], v9 offset:64",
        "\ts_waitcnt lgkmcnt(1)", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[0:3], a[0:3]", "\tds_read_b128 v[0:3], v9",
        "\ts_waitcnt vmcnt(2) lgkmcnt(0)", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[4:7], v[0:3], a[0:3]", "\tv_add_u32 v9, v9, v8",
        "\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm", ".Lfunc_end0:", "; NumVgprs: 10", "; NumAgprs: 4", "; ScratchSize: 0", ""])
    (k,) = A.audit(asm)
    assert (k["name"], k["vgpr"], k["agpr"], k["scratch"]) == ("k", 10, 4, 0)
    (loop,) = k["loops"]
    assert loop["text"] == "Bdrr |1| Mr |v2,0| M"
    assert (loop["mfma"], loop["reads"], loop["exposed"]) == (2, 3, 1)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc is not installed")
def test_ring_kernel_reads_one_step_ahead_of_its_mfmas():
    A = _tool()
    asm = A.compile_to_asm(os.path.join(ROOT, "unet-convlstm_amd", "csrc", "igemm_fwd.hip"), f16=False)
    ks = [k for k in A.audit(asm, "igemm_fwd_c64_kernel")]
    assert len(ks) == 1
    k = ks[0]
    print(A.report(asm, "igemm_fwd_c64_kernel"))
    assert k["scratch"] == 0
    assert k["vgpr"] + k["agpr"] <= 512
    loops = [l for l in k["loops"] if l["mfma"] == 288]
    assert len(loops) == 1, "the tile loop: 18 steps x 16 MFMAs, once"
    ev = loops[0]["events"]
    kinds = [e if isinstance(e, str) else e.kind for e in ev]
    first_m = kinds.index("M")
    stream = A.mfma_stream(ev)              # the tile's opening barrier ... its last MFMA (no LDS read follows: the epilogue is registers)
    assert stream[0].kind == "B"
    assert sum(1 for e in stream if not isinstance(e, str) and e.kind == "r") == 144
    # at most two waits for everything that directly follow a read (today's code: step 0, and none in the tail)
    exposed = A.exposed_reads(stream)
    assert len(exposed) <= 2, f"{len(exposed)} read-then-lgkmcnt(0) in the tile: " + A.render(stream)
    assert len(A.exposed_reads(ev)) == len(exposed)
    # one vmcnt(0) and one barrier open the MFMA stream: the barrier that starts `stream` is preceded by the vmcnt(0) wait
    # (the row-issue loops between them hold no event of their own), and nothing but the prefetch and reads lies between it and the MFMAs
    head = [e for e in ev[:first_m] if not isinstance(e, str)]
    opening = max(i for i, e in enumerate(head) if e.kind == "B")
    assert head[opening - 1].kind == "w" and head[opening - 1].vm == 0
    assert all(e.kind == "r" or (e.kind == "w" and e.vm is None) for e in head[opening + 1:])
    # exactly as many barriers and vmcnt waits in front of the stream as the source has: the conditional barrier of an image
    # boundary, then vmcnt(0) + barrier (the compiler may emit the asm wait next to one of its own)
    assert sum(1 for e in head if e.kind == "B") == 2
    assert all(e.vm == 0 for e in head if e.kind == "w" and e.vm is not None)
    # no vmcnt wait inside the MFMA stream: the next tile's rows stay in flight
    assert not [e for e in stream[1:] if not isinstance(e, str) and e.kind == "w" and e.vm is not None]
    first_r = next(i for i, e in enumerate(stream) if not isinstance(e, str) and e.kind == "r")
    assert not [e for e in stream[first_r:] if isinstance(e, str) or e.kind in "Bd"], "a barrier, DMA or inner loop inside the MFMA stream"
