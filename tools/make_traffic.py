#!/usr/bin/env python3
"""profiles/traffic.json from two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) of bench.py.
usage: tools/make_traffic.py <fetch counter_collection.csv> <write counter_collection.csv>
Counter unit = KiB; FETCH_SIZE is doubled (gfx950 counts 128-B read requests as 64 B,
MI355X_MICROARCH.md 'HBM'); per-launch averages, first launch of each kernel dropped."""
import collections
import csv
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def per_kernel(path, counter):
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] != counter:
            continue
        m = re.search(r"(k_[a-z_]+)", r["Kernel_Name"])
        name = m.group(1) if m else "?"
        if name == "k_zipper_cols":                                  # k_zipper_cols<T, W, HY, COPY, GEN>: the copy probe has COPY = true
            targs = r["Kernel_Name"].split("k_zipper_cols<")[1].split(">")[0].replace(" ", "").split(",")
            if len(targs) > 3 and targs[3] == "true":
                name = "k_zipper_cols_copy_probe"
        acc[name].append(float(r["Counter_Value"]))
    return {k: sum(v[1:]) / max(1, len(v[1:])) * 1024.0 for k, v in acc.items()}


def main():
    fetch, write = per_kernel(sys.argv[1], "FETCH_SIZE"), per_kernel(sys.argv[2], "WRITE_SIZE")
    sys.path.insert(0, ROOT)
    from bench_common import sources_sha16
    csrc = "orthogonalsphericalshellgrids.jl_amd/csrc/"
    grid_src = [csrc + f for f in ("tpg_grid.hip", "tpg_batch.hpp", "tpg_math.hpp", "tpg_tiles.hpp")]
    # the launch layer is part of the key: launch geometry decides traffic as much as kernel text does
    fill_src = [csrc + f for f in ("tpg_zipper_kernels.hpp", "tpg_launch.hpp", "tpg_zipper.hip")]
    sources = {"k_tables": grid_src, "k_cells_tile": grid_src, "k_cells": grid_src, "k_halos": grid_src, "k_south": grid_src,
               "k_fill_merged": fill_src, "k_zipper_cols": fill_src, "k_periodic_x_vec": fill_src, "k_fill_fused_vec": fill_src,
               "k_zipper_cols_copy_probe": fill_src, "k_pack": fill_src, "k_synthetic": [csrc + "tpg_testabi.hip"]}
    kernels = {}
    for k in fetch:
        # bench.py reports a kernel's `traffic` only while the files that kernel is compiled from hash to what they were when measured
        kernels[k] = {"fetch_bytes_raw": fetch[k], "fetch_bytes_corrected": 2 * fetch[k], "write_bytes": write.get(k, 0.0),
                      "hbm_bytes_per_launch": 2 * fetch[k] + write.get(k, 0.0),
                      "sources": sources.get(k, []), "sources_sha16": sources_sha16(sources[k]) if k in sources else None}
    out = {"_source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, tools/pmc.sh) over `bench.py --full --no-aux --no-fill-step "
                      f"--steps 5 --warmup 1`: {os.path.relpath(sys.argv[1], ROOT)}, {os.path.relpath(sys.argv[2], ROOT)}; per-launch averages "
                      "(first launch dropped). Counter unit = KiB; FETCH_SIZE doubled (gfx950 counts 128-B read requests as 64 B, "
                      "MI355X_MICROARCH.md 'HBM'); WRITE_SIZE as read.",
           "kernels": kernels}
    with open(os.path.join(ROOT, "profiles", "traffic.json"), "w") as f:
        json.dump(out, f, indent=1)
    for k, v in kernels.items():
        print(f"{k:20s} {v['hbm_bytes_per_launch'] / 1e6:10.2f} MB per launch")


if __name__ == "__main__":
    main()
