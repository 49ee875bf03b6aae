#!/usr/bin/env python3
"""Static prologue of the tile kernel: what k_cells_tile<double, true, 8> and <float, true, 8> hold between their entry and their first
v_mul_f64, counted by class, with every load and every s_waitcnt in the order of the listing.  Compiles csrc/tpg_grid.hip to gfx950
assembly with the flags of csrc/Makefile (the product's code: no -DTPG_CELLS_NO_FALLBACK), or reads an assembly file.  A static count of
the listing, branches not taken included -- at the flagship size no lane takes wrap_col's generic modulo, and the general path of row Ny
starts behind the last wait.  Needs hipcc, no GPU.

usage: tools/cells_prologue.py [--csrc DIR] [--flags '...'] [--asm FILE] [--label TEXT] [--list | --counts]     (output: stdout)"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cells_ledger import KERNELS, ROOT, makefile_vars   # noqa: E402


def prologue(asm, key):
    """instruction lines (comments stripped) of the one function whose name holds `key`, up to its first v_mul_f64"""
    out, inside, hits = [], False, 0
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            inside = key in m.group(1)
            hits += inside
            continue
        if not inside:
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        if t.startswith("v_mul_f64"):
            inside = False
            continue
        out.append(t)
    if hits != 1:
        sys.exit(f"{hits} functions match {key}")
    return out


def classify(op):
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar load"
    if op.startswith(("global_load", "flat_load", "buffer_load")):
        return "global load"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("s_cbranch", "s_branch", "s_swappc", "s_setpc")):
        return "branch"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc"))
    ap.add_argument("--flags", default="", help="extra compiler flags, as GRID_FLAGS of the Makefile")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("--label", default="")
    ap.add_argument("--list", action="store_true", help="print the whole prologue, not only its loads and waits")
    ap.add_argument("--counts", action="store_true", help="print the counts only")
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        hipcc, flags = makefile_vars(a.csrc)
        with tempfile.TemporaryDirectory() as d:
            s = os.path.join(d, "tpg_grid.s")
            r = subprocess.run([hipcc] + flags + a.flags.split() + ["--cuda-device-only", "-S", "-o", s, os.path.join(a.csrc, "tpg_grid.hip")],
                               capture_output=True, text=True)
            if r.returncode:
                sys.exit(r.stderr[-4000:])
            asm = open(s).read()
    if a.label:
        print(f"== {a.label}")
    for shown, key in KERNELS:
        lines = prologue(asm, key)
        n = collections.Counter(classify(t.split()[0]) for t in lines)
        print(f"{shown}: {len(lines)} instructions from the entry to the first v_mul_f64: " + ", ".join(f"{k} {v}" for k, v in sorted(n.items())))
        if a.counts or key != KERNELS[0][1]:          # the listing of the Float64 kernel only: the Float32 one differs by an instruction
            continue
        for k, t in enumerate(lines):
            if a.list or classify(t.split()[0]) in ("s_waitcnt", "scalar load", "global load", "LDS", "branch"):
                print(f"  {k:4d}  {t}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
