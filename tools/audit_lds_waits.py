#!/usr/bin/env python3
"""Code-object audit of the LDS read / wait / MFMA interleaving of a csrc file.

    python tools/audit_lds_waits.py unet-convlstm_amd/csrc/igemm_fwd.hip [--f16] [--kernel SUBSTRING] [--asm FILE.s]

Compiles the file to gfx950 assembly with build.py's own flags (`hipcc -S --cuda-device-only`: no GPU is needed) and
prints, per kernel that holds MFMAs, the loops whose own body issues MFMAs as one string:

    M      v_mfma*
    r      ds_read*
    |n|    s_waitcnt lgkmcnt(n)        |vN|  s_waitcnt vmcnt(N)        |vN,n|  both counters in one instruction
    B      s_barrier
    d      buffer_load ... lds (LDS-DMA)
    {..}   a nested loop (printed on its own if it holds MFMAs)

together with the VGPR / AGPR counts, the scratch bytes, and per loop the number of EXPOSED reads: an `lgkmcnt(0)` wait
whose nearest preceding `r` or `M` is an `r` -- the wave issued a read and at once waits for everything, so the whole
LDS round trip is idle time unless another wave of the SIMD fills it.

Only those five kinds of lines and the resource comments are read; everything else of the assembly is ignored.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unet-convlstm_amd")

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.L\w+)")
_CNT = re.compile(r"(vmcnt|lgkmcnt)\((\d+)\)")
_RES = re.compile(r"^; (NumVgprs|NumAgprs|ScratchSize): (\d+)")


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return shutil.which("hipcc")


def compile_to_asm(src: str, f16: bool = False) -> str:
    """The gfx950 device assembly of one csrc file, with the flags the library is built with."""
    spec = importlib.util.spec_from_file_location("uclstm_build", os.path.join(PKG, "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    cc = hipcc()
    if not cc:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "a.s")
        cmd = [cc, *B.FLAGS, *(B.F16_FLAGS if f16 else []), f"-I{os.path.dirname(os.path.abspath(B.HEADER))}", "-Wno-unused-command-line-argument",
               "-S", "--cuda-device-only", os.path.abspath(src), "-o", out]
        subprocess.run(cmd, check=True)
        with open(out) as f:
            return f.read()


class Event:
    __slots__ = ("kind", "vm", "lgkm", "line")

    def __init__(self, kind, line, vm=None, lgkm=None):
        self.kind, self.line, self.vm, self.lgkm = kind, line, vm, lgkm

    def __str__(self):
        if self.kind != "w":
            return self.kind
        if self.vm is None:
            return f"|{self.lgkm}|"
        return f"|v{self.vm}|" if self.lgkm is None else f"|v{self.vm},{self.lgkm}|"


def _classify(text: str, line: int):
    op = text.split(None, 1)[0] if text.split() else ""
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return Event("M", line)
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return Event("r", line)
    if op == "s_barrier":
        return Event("B", line)
    if op.startswith("buffer_load") and re.search(r"\blds\b", text):
        return Event("d", line)
    if op == "s_waitcnt":
        c = {k: int(v) for k, v in _CNT.findall(text)}
        if c:
            return Event("w", line, c.get("vmcnt"), c.get("lgkmcnt"))
    return None


def parse(asm: str):
    """[{name, vgpr, agpr, scratch, items}]: items is the kernel's instruction stream reduced to Events, labels
    ('L', name) and branches ('J', target), in program order."""
    kernels, cur = [], None
    funcs = set(re.findall(r"^\s+\.type\s+([\w.$]+),@function", asm, re.M))
    for ln, raw in enumerate(asm.splitlines(), 1):
        m = _LABEL.match(raw)
        if m:
            name = m.group(1)
            if name in funcs:
                cur = {"name": name, "vgpr": None, "agpr": None, "scratch": None, "items": [], "open": True}
                kernels.append(cur)
            elif cur is not None and cur["open"]:
                if name.startswith(".Lfunc_end"):
                    cur["open"] = False
                else:
                    cur["items"].append(("L", name))
            continue
        if cur is None:
            continue
        m = _RES.match(raw)
        if m:
            cur[{"NumVgprs": "vgpr", "NumAgprs": "agpr", "ScratchSize": "scratch"}[m.group(1)]] = int(m.group(2))
            continue
        if not cur["open"] or not raw.startswith("\t") or raw.startswith("\t."):
            continue
        text = raw.split(";", 1)[0].strip()
        m = _BRANCH.match(raw)
        if m:
            cur["items"].append(("J", m.group(1)))
            continue
        ev = _classify(text, ln)
        if ev is not None:
            cur["items"].append(("E", ev))
    for k in kernels:
        del k["open"]
    return kernels


def loops(kernel):
    """Natural loops by backward branches: [(first, last)] item index ranges, outer loops first."""
    pos = {v: i for i, (t, v) in enumerate(kernel["items"]) if t == "L"}
    spans = {}
    for i, (t, v) in enumerate(kernel["items"]):
        if t == "J" and v in pos and pos[v] < i:
            spans[pos[v]] = max(spans.get(pos[v], 0), i)
    return sorted(spans.items(), key=lambda s: (s[0], -s[1]))


def own_events(kernel, span, all_spans):
    """The events of a loop in program order; a nested loop is replaced by the marker string '{..}'."""
    inner = [s for s in all_spans if s != span and span[0] <= s[0] and s[1] <= span[1]]
    out, i = [], span[0]
    while i <= span[1]:
        hit = [s for s in inner if s[0] == i]
        if hit:
            out.append("{..}")
            i = max(s[1] for s in hit) + 1
            continue
        t, v = kernel["items"][i]
        if t == "E":
            out.append(v)
        i += 1
    return out


def exposed_reads(events):
    """The `lgkmcnt(0)` waits whose nearest preceding read or MFMA is a read."""
    hits, last = [], None
    for e in events:
        if isinstance(e, str):
            last = None
        elif e.kind in "Mr":
            last = e.kind
        elif e.kind == "w" and e.lgkm == 0 and last == "r":
            hits.append(e)
    return hits


def render(events) -> str:
    out, prev = [], None
    for e in events:
        s = str(e)
        if prev is not None and (s[0] == "|" or prev[0] == "|" or s == "{..}" or prev == "{..}"):
            out.append(" ")
        out.append(s)
        prev = s
    return "".join(out)


def mfma_stream(events):
    """The slice of a loop body from its last barrier in front of the first MFMA through the last MFMA."""
    ms = [i for i, e in enumerate(events) if not isinstance(e, str) and e.kind == "M"]
    if not ms:
        return []
    start = 0
    for i in range(ms[0] - 1, -1, -1):
        if not isinstance(events[i], str) and events[i].kind == "B":
            start = i
            break
    return events[start:ms[-1] + 1]


def audit(asm: str, only: str | None = None):
    """[{name, vgpr, agpr, scratch, loops: [{events, text, mfma, reads, exposed}]}] for the kernels that hold MFMAs."""
    res = []
    for k in parse(asm):
        if only and only not in k["name"]:
            continue
        spans = loops(k)
        ls = []
        for sp in spans:
            ev = own_events(k, sp, spans)
            n_m = sum(1 for e in ev if not isinstance(e, str) and e.kind == "M")
            if n_m:
                ls.append({"events": ev, "text": render(ev), "mfma": n_m, "reads": sum(1 for e in ev if not isinstance(e, str) and e.kind == "r"),
                           "exposed": len(exposed_reads(ev))})
        if ls or only:
            res.append({"name": k["name"], "vgpr": k["vgpr"], "agpr": k["agpr"], "scratch": k["scratch"], "loops": ls})
    return res


def demangled(names):
    tool = shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def report(asm: str, only: str | None = None, width: int = 116) -> str:
    ks = audit(asm, only)
    nice = demangled([k["name"] for k in ks])
    out = []
    for k in ks:
        out.append(f"{nice[k['name']]}")
        out.append(f"  VGPR {k['vgpr']}  AGPR {k['agpr']}  scratch {k['scratch']} B")
        for i, l in enumerate(k["loops"]):
            out.append(f"  loop {i}: {l['mfma']} MFMA, {l['reads']} ds_read, {l['exposed']} read-then-lgkmcnt(0)")
            words, line = l["text"].split(" "), "    "
            for w in words:
                while len(line) + len(w) > width and len(line) > 4:
                    out.append(line.rstrip())
                    line = "    "
                while len(w) > width - 4:
                    out.append("    " + w[:width - 4])
                    w = w[width - 4:]
                line += w + " "
            if line.strip():
                out.append(line.rstrip())
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("source", nargs="?", help="a csrc file (compiled here) -- or give --asm")
    ap.add_argument("--f16", action="store_true", help="the -DUCLSTM_ACT_F16 pass")
    ap.add_argument("--kernel", help="only kernels whose (mangled) name contains this")
    ap.add_argument("--asm", help="audit this assembly file instead of compiling")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            asm = f.read()
    elif a.source:
        asm = compile_to_asm(a.source, a.f16)
    else:
        ap.error("a source file or --asm")
    print(report(asm, a.kernel))


if __name__ == "__main__":
    main()
