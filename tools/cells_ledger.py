#!/usr/bin/env python3
"""Static main-path ledger of the tile kernel: compiles csrc/tpg_grid.hip to gfx950 assembly with -DTPG_CELLS_NO_FALLBACK=1 (no batch
function reports a rare argument, so every scalar fallback is dead code and the compiler deletes it) and with the flags of csrc/Makefile,
and prints the VALU opcode histogram of k_cells_tile<double, true, 8> and <float, true, 8> before and after the block barrier.

Instructions are counted by opcode class only (the encoding suffix _e32 / _e64 / _dpp / _sdwa is dropped); both phase-2 branches and both
`lsmall` branches are in the count: it is a static count of the generated code, not of what a wave executes.  Needs hipcc, no GPU.

usage: tools/cells_ledger.py [--csrc DIR] [--flags '...'] [--label TEXT] [--keep-asm FILE]     (output: stdout)"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = (("k_cells_tile<double, true, 8>", "k_cells_tileIdLb1ELi8E"), ("k_cells_tile<float, true, 8>", "k_cells_tileIfLb1ELi8E"))
FP64 = ("v_add_f64", "v_mul_f64", "v_fma_f64", "v_fmac_f64")


def makefile_vars(csrc):
    """HIPCC, ARCH and CXXFLAGS as csrc/Makefile sets them (environment overrides HIPCC / ARCH, as in make)"""
    v = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"^(HIPCC|ARCH|CXXFLAGS)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m and m.group(1) not in v:
            v[m.group(1)] = m.group(2).strip()
    hipcc, arch = os.environ.get("HIPCC", v["HIPCC"]), os.environ.get("ARCH", v["ARCH"])
    return hipcc, v["CXXFLAGS"].replace("$(ARCH)", arch).split()


def kernel_bodies(asm):
    """{mangled name: instruction lines} of the functions of an assembly file"""
    out, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        if name is None:
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out[name].append(t.split()[0])
    return out


def opclass(op):
    return re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", op)


def ledger(ops):
    """(histogram before the barrier, histogram after it) of the VALU instructions"""
    cut = ops.index("s_barrier") if "s_barrier" in ops else len(ops)
    return [collections.Counter(opclass(o) for o in part if o.startswith("v_")) for part in (ops[:cut], ops[cut:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc"))
    ap.add_argument("--flags", default="", help="extra compiler flags, as GRID_FLAGS of the Makefile")
    ap.add_argument("--label", default="")
    ap.add_argument("--keep-asm", default=None)
    a = ap.parse_args()
    hipcc, flags = makefile_vars(a.csrc)
    with tempfile.TemporaryDirectory() as d:
        s = a.keep_asm or os.path.join(d, "tpg_grid.s")
        cmd = [hipcc] + flags + a.flags.split() + ["-DTPG_CELLS_NO_FALLBACK=1", "--cuda-device-only", "-S", "-o", s, os.path.join(a.csrc, "tpg_grid.hip")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr[-4000:])
        bodies = kernel_bodies(open(s).read())
    if a.label:
        print(f"== {a.label}")
    for shown, key in KERNELS:
        names = [n for n in bodies if key in n]
        if len(names) != 1:
            sys.exit(f"{shown}: {len(names)} functions match {key}")
        before, after = ledger(bodies[names[0]])
        total = before + after
        nb, na = sum(before.values()), sum(after.values())
        f64 = sum(total[o] for o in FP64)
        print(f"{shown}: static main-path VALU {nb + na} = {nb} before s_barrier + {na} after; FP64 add/mul/fma/fmac {f64}, "
              f"v_rcp_f64 {total['v_rcp_f64']}, v_rsq_f64 {total['v_rsq_f64']}, the rest {nb + na - f64 - total['v_rcp_f64'] - total['v_rsq_f64']}")
        print(f"  {'opcode':<22}{'before':>8}{'after':>8}{'total':>8}")
        for op, n in sorted(total.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"  {op:<22}{before[op]:>8}{after[op]:>8}{n:>8}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
