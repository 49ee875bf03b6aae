"""isa_diff.py -- compare the gfx950 code objects of two builds of the HIP objects, kernel by kernel.

    python tools/isa_diff.py OLD_DIR NEW_DIR [name.o ...]

OLD_DIR / NEW_DIR hold the objects of csrc/ (e.g. a copy of csrc/*.o taken at the parent commit, and csrc/ itself).  For every
object (default: every *.o in OLD_DIR) the device code object is taken out of the .hip_fatbin section (llvm-objcopy +
clang-offload-bundler), disassembled (llvm-objdump -d) and compared per kernel symbol, together with the kernel's descriptor metadata
(llvm-readelf --notes: register counts, spills, LDS, scratch and kernarg size).  Kernels are paired by symbol first.  A kernel of OLD_DIR
whose symbol is gone is then paired by content (pair_renamed): if its disassembly and its descriptor entries both equal those of exactly
one kernel that only NEW_DIR has, the two are one kernel under a new name (a changed template parameter or argument type) and are
reported under `renamed`, old -> new; n identical kernels against n identical kernels pair in symbol order.  Prints one JSON line: per
object, whether the code objects are byte-identical, the renamed pairs, the kernels whose disassembly or metadata differs, and those that
exist on one side only (`only_old`, `only_new`: what no pairing took); exit status 0 only if nothing differs and nothing is left on one
side.  `code_object_identical` stays a byte comparison of the whole code objects: a rename changes the symbol table, so it is false for
an object with a renamed kernel even when nothing else moved."""
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def has_device_code(obj):
    out = subprocess.run([f"{LLVM}/llvm-objdump", "-h", obj], capture_output=True, text=True, check=True).stdout
    return ".hip_fatbin" in out


def code_object(obj, tmp):
    fatbin = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fatbin}", obj, os.path.join(tmp, "discard.o")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fatbin}", f"--output={co}",
                    "--unbundle"], check=True)
    with open(co, "rb") as f:
        return co, f.read()


def kernels(co):
    """symbol -> disassembly lines without addresses / encodings"""
    out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                         capture_output=True, text=True, check=True).stdout
    syms, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            cur = m.group(1)
            syms[cur] = []
        elif cur and line.strip():
            syms[cur].append(re.sub(r"//.*$", "", line).strip())
    return syms


DESCRIPTOR = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
              "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def descriptors(co):
    """symbol -> the DESCRIPTOR entries of its amdhsa.kernels record"""
    out = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    recs, cur = [], None
    for line in out.splitlines():
        m = re.match(r"^(  - |    )\.(\w+):\s+(\S.*)$", line)           # scalar entries of a kernel record (its .args are nested deeper)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
            recs.append(cur)
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip()
    return {r["name"]: {k: r.get(k) for k in DESCRIPTOR} for r in recs if "name" in r}


def pair_renamed(lines_old, lines_new, desc_old, desc_new):
    """(renamed, only_old, only_new) for two builds' symbol -> disassembly lines and symbol -> descriptor dictionaries.  Among the symbols
    only one build has, kernels of equal content (the same lines and the same descriptor) form a group.  A group with ONE kernel on each
    side is a rename.  So is a group with the same number n > 1 on both sides -- instantiations that compile to the same code, such as
    the aligned and the element-aligned form of a chunk type: they are paired in symbol order, and which twin is which cannot matter,
    every one has a partner of equal content.  A group with unequal numbers (one old kernel and two identical candidates, a kernel
    missing on one side) pairs nothing: its kernels stay in only_old / only_new"""
    groups = {}
    for side, lines, desc, other in ((0, lines_old, desc_old, lines_new), (1, lines_new, desc_new, lines_old)):
        for k in sorted(set(lines) - set(other)):
            key = (tuple(lines[k]), tuple(sorted((desc.get(k) or {}).items())))
            groups.setdefault(key, ([], []))[side].append(k)
    renamed, only_old, only_new = {}, [], []
    for old, new in groups.values():
        if len(old) == len(new):
            renamed.update(zip(old, new))
        else:
            only_old += old
            only_new += new
    return dict(sorted(renamed.items())), sorted(only_old), sorted(only_new)


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    names = sys.argv[3:] or sorted(n for n in os.listdir(old_dir) if n.endswith(".o"))
    report = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            if not has_device_code(os.path.join(old_dir, n)):
                report[n] = {"device_code": False}
                continue
            os.makedirs(os.path.join(tmp, "old"), exist_ok=True)
            os.makedirs(os.path.join(tmp, "new"), exist_ok=True)
            co_a, a = code_object(os.path.join(old_dir, n), os.path.join(tmp, "old"))
            co_b, b = code_object(os.path.join(new_dir, n), os.path.join(tmp, "new"))
            ka, kb = kernels(co_a), kernels(co_b)
            da, db = descriptors(co_a), descriptors(co_b)
            assert da and set(da) <= set(ka), "kernel metadata of " + n + " not understood"
            renamed, only_old, only_new = pair_renamed(ka, kb, da, db)
            report[n] = {"code_object_identical": a == b, "kernels": len(ka), "descriptors": len(da),
                         "differing": sorted(k for k in ka if k in kb and ka[k] != kb[k]),
                         "metadata_differing": sorted(k for k in ka if k in kb and da.get(k) != db.get(k)),
                         "renamed": renamed, "only_old": only_old, "only_new": only_new}
    print(json.dumps(report))
    bad = ("differing", "metadata_differing", "only_old", "only_new")
    return 0 if all(not any(r.get(k) for k in bad) for r in report.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
