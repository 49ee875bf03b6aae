"""bench_immersed.py -- the immersed-boundary mask pass (tpg_mask_immersed_fields) on a model's (u, v, w, T, S).

3600 x 1800 x 75, z = (-1, 0), halo 4 and (5, 5, 5), Float64 and Float32, two grid-fitted bottoms, both functions of (lambda, phi) only:
  A  the reference's (examples/bickley_jet.jl:25-29): h = 0 in the two 5-degree pole boxes and for phi < -78, h = -1 elsewhere -- whole
     columns, a few per cent of the cells;
  B  h = -clip(0.5 + 0.5 sin 3 lambda cos 2 phi + 0.2 cos 5 lambda sin 4 phi, 0, 1) with A's boxes on top -- about half of the cells.
Per case: the masked cells of the five fields (counted from the grid's count planes), the algorithmic bytes (masked cells x sizeof(T) +
4 Nx Ny per field for its count plane), and -- in ONE process, alternating within every repetition, each call cold (after a 1 GiB read-only
pass), stream-event brackets --
  * mask_ms        the ImmersedMaskPlan call (one launch per geometry group: u, v, T, S together, w alone);
  * flat_ms        a flat device fill (torch zero_) of the same number of bytes: the yardstick of the sibling benches;
  * where_ms       an in-place torch masked_fill_ (= where(mask, value, field)) over the interior of the same fields: what an every-cell pass moves;
  * fill_ms        the plain HaloFillPlan of the five fields (what the parent commit runs);
  * mask_fill_ms   halo_fill_plan(fields, mask_immersed=0.0): the mask launches in front of that fill.
Runnable alone:  python bench_immersed.py [--only SUBSTRING] [--product-lib PATH]   -> one JSON line  (PATH: another build of the product
library, e.g. one with -DTPG_IMMERSED_NT=1, for an A/B in two runs of the same command).
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
REPS, DROP = 22, 2
SIZE = (3600, 1800, 75)


def _boxes(torch, lam, phi):
    return (((lam - 70).abs() < 5) & ((55 - phi).abs() < 5)) | (((lam - 250).abs() < 5) & ((55 - phi).abs() < 5)) | (phi < -78)


def bottom_a(torch):
    return lambda lam, phi: torch.where(_boxes(torch, lam, phi), torch.zeros_like(lam), -torch.ones_like(lam))


def bottom_b(torch):
    def h(lam, phi):
        rl, rp = torch.deg2rad(lam), torch.deg2rad(phi)
        b = -(0.5 + 0.5 * torch.sin(3 * rl) * torch.cos(2 * rp) + 0.2 * torch.cos(5 * rl) * torch.sin(4 * rp)).clamp(0, 1)
        return torch.where(_boxes(torch, lam, phi), torch.zeros_like(b), b)
    return h


def run_case(torch, osg, _lib, dev, size, h, tdt, which):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-1, 0))
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom((bottom_a if which == "A" else bottom_b)(torch)))
    nf, per, imp = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition, osg.ImpenetrableBoundaryCondition
    Ce, Fa = osg.Center, osg.Face
    specs = [("u", (Fa, Ce, Ce), "fc", dict(south=nf(), bottom=nf(), top=nf())), ("v", (Ce, Fa, Ce), "cf", dict(south=imp(), bottom=nf(), top=nf())),
             ("w", (Ce, Ce, Fa), "cc", dict(south=nf(), bottom=imp(), top=imp())), ("T", (Ce, Ce, Ce), "cc", dict(south=nf(), bottom=nf(), top=nf())),
             ("S", (Ce, Ce, Ce), "cc", dict(south=nf(), bottom=nf(), top=nf()))]
    fs, masks, masked = [], [], 0
    lev = torch.arange(1, nz + 1, device=dev, dtype=torch.int32)[:, None, None]
    counts = ibg.column_counts
    for name, loc, key, sides in specs:
        f = osg.Field(loc, ibg, name=name, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))
        f.data.uniform_(0.5, 1.5)
        fs.append(f)
        n = counts[key]
        m = lev <= ((n + 1).clamp(max=nz) if loc[2] is Fa else n)[None]              # the every-cell pass's mask over levels 1..Nz of the grid
        masks.append(m)
        masked += int(m.sum())
    columns = int((counts["cc"] == nz).sum())
    nbytes = masked * esz + len(fs) * 4 * nx * ny
    mask_plan = osg.immersed_mask_plan(fs, 0.0)
    fill_plan = osg.halo_fill_plan(fs)
    both_plan = osg.halo_fill_plan(fs, mask_immersed=0.0)
    flat_buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def where():
        for f, m in zip(fs, masks):
            inner = f.data[hz:hz + nz, hy:hy + ny, hx:hx + nx]
            inner.masked_fill_(m, 0)                                       # one read and one write of every interior cell, no temporary

    runs = {"mask_ms": mask_plan, "flat_ms": flat_buf.zero_, "where_ms": where, "fill_ms": fill_plan, "mask_fill_ms": both_plan}
    for fn in runs.values():                                               # warm: code objects, first-call queries, the allocator
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(REPS):
        for k, fn in runs.items():                                         # alternating: every repetition times each of them once
            flush.sum()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    t = {k: statistics.median(v[DROP:]) for k, v in times.items()}
    spread = {k.replace("_ms", "_min_max_ms"): [min(v[DROP:]), max(v[DROP:])] for k, v in times.items()}
    for f, m, (name, _, key, _) in zip(fs, masks, specs):                  # what was timed is the mask: every masked cell is 0
        assert bool(((f.data[hz:hz + nz, hy:hy + ny, hx:hx + nx] == 0) | ~m).all()), name
    frac = lambda ms: nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
    where_bytes = sum(2 * nx * ny * nz * esz + nx * ny * nz for _ in fs)
    out = {"bottom": which, "size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32", "fields": [s[0] for s in specs],
           "masked_cells": masked, "masked_share_of_cells": masked / (len(fs) * nx * ny * nz), "land_columns": columns,
           "land_share_of_columns": columns / (nx * ny), "algorithmic_bytes": nbytes, "where_bytes": where_bytes, **t, **spread,
           "mask_frac_of_hbm_peak": frac(t["mask_ms"]), "flat_frac_of_hbm_peak": frac(t["flat_ms"]),
           "mask_over_flat_time": t["mask_ms"] / t["flat_ms"], "mask_over_where_time": t["mask_ms"] / t["where_ms"],
           "mask_fill_minus_fill_ms": t["mask_fill_ms"] - t["fill_ms"]}
    del mask_plan, fill_plan, both_plan, fs, masks, ibg, grid, flat_buf, flush, counts
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def bench_immersed(torch, osg, _lib, dev, only=""):
    out = {}
    for which in ("A", "B"):
        for h in (4, 5):
            for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                name = f"{which}_halo{h}_{tag}"
                if only in name:
                    out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, which)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped; within every repetition the five calls are timed one after the other, each cold "
                     "(after a 1 GiB read-only pass), by a stream-event bracket; mask_ms = the ImmersedMaskPlan call (two launches); flat_ms = "
                     "torch zero_ of algorithmic_bytes; where_ms = in-place torch masked_fill_ over the interior of the five fields (where_bytes: a "
                     "read and a write of every interior cell plus one mask byte); fill_ms / mask_fill_ms = the HaloFillPlan without / with "
                     "mask_immersed=0.0; fractions of 8 TB/s over algorithmic_bytes = masked cells x sizeof(T) + 4 Nx Ny per field")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    if "--product-lib" in sys.argv:
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--product-lib") + 1])
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_immersed(torch, osg, _lib, dev, only)
    out["product_library"] = os.path.relpath(_lib.LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
