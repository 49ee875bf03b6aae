"""isa_diff.py -- compare the gfx950 code objects of two builds of the HIP objects, kernel by kernel.

    python tools/isa_diff.py OLD_DIR NEW_DIR [name.o ...]

OLD_DIR / NEW_DIR hold the objects of csrc/ (e.g. a copy of csrc/*.o taken at the parent commit, and csrc/ itself).  For every
object (default: every *.o in OLD_DIR) the device code object is taken out of the .hip_fatbin section (llvm-objcopy +
clang-offload-bundler), disassembled (llvm-objdump -d) and compared per kernel symbol.  Prints one JSON line: per object, whether
the code objects are byte-identical and the kernels whose disassembly differs or that exist on one side only."""
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
            report[n] = {"code_object_identical": a == b, "kernels": len(ka),
                         "differing": sorted(k for k in ka if k in kb and ka[k] != kb[k]),
                         "only_old": sorted(set(ka) - set(kb)), "only_new": sorted(set(kb) - set(ka))}
    print(json.dumps(report))
    return 0 if all(not r.get("differing") and not r.get("only_old") for r in report.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
