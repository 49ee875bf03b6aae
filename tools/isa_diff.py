"""isa_diff.py -- compare the gfx950 code objects of two builds of the HIP objects, kernel by kernel.

    python tools/isa_diff.py OLD_DIR NEW_DIR [name.o ...]

OLD_DIR / NEW_DIR hold the objects of csrc/ (e.g. a copy of csrc/*.o taken at the parent commit, and csrc/ itself).  For every
object (default: every *.o in OLD_DIR) the device code object is taken out of the .hip_fatbin section (llvm-objcopy +
clang-offload-bundler), disassembled (llvm-objdump -d) and compared per kernel symbol, together with the kernel's descriptor metadata
(llvm-readelf --notes: register counts, spills, LDS, scratch and kernarg size).  Prints one JSON line: per object, whether the code
objects are byte-identical and the kernels whose disassembly or metadata differs or that exist on one side only; exit status 0 only
if there is none of either."""
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
            report[n] = {"code_object_identical": a == b, "kernels": len(ka), "descriptors": len(da),
                         "differing": sorted(k for k in ka if k in kb and ka[k] != kb[k]),
                         "metadata_differing": sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k)),
                         "only_old": sorted(set(ka) - set(kb)), "only_new": sorted(set(kb) - set(ka))}
    print(json.dumps(report))
    bad = ("differing", "metadata_differing", "only_old", "only_new")
    return 0 if all(not any(r.get(k) for k in bad) for r in report.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
