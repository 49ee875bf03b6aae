"""bench_bounded.py -- the no-flux south / bottom / top halo fill (tpg_fill_bounded_halos) of a model's default fields.

Every HydrostaticFreeSurfaceModel field carries a no-flux condition on each bounded side where it sits at Center: bottom and top for
c, u, v and zeta, south for the y-Center fields c and u.  After the horizontal fill (zipper -> periodic x, one merged launch) the
library mirrors those halos in one more launch.  This script times, per case:

  * fill_ms     -- the whole default-field fill: a stream-event bracket around the HaloFillPlan call (every launch it makes);
  * bounded_ms  -- the bounded pass alone: a stream-event bracket around its one tpg_fill_bounded_halos call (one launch);
  * bounded_algorithmic_bytes = 2 x cells written x sizeof(T), and its fraction of 8 TB/s;
  * copy_ms     -- beside it, a flat device copy (torch copy_) of the same number of bytes, timed the same way.

Cases: 3600 x 1800 x 75 at halo 4 and (5, 5, 5), Float64 and Float32; config 5, 8640 x 4320 x 100 at halo 5 in Float64 with as many
fields as fit comfortably (peak device memory recorded).  Each figure: median of 10 after 2 dropped, cold (after a 1 GiB read-only pass).
Runnable alone:  python bench_bounded.py [--no-config5]   -> one JSON line.
"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
SOUTH, BOTTOM, TOP = 1, 2, 4
MODEL = [("c", 0, 0, SOUTH | BOTTOM | TOP), ("u", 1, 0, SOUTH | BOTTOM | TOP), ("v", 0, 1, BOTTOM | TOP), ("zeta", 1, 1, BOTTOM | TOP)]
REPS, DROP = 12, 2


def bounded_cells(size, halo, sides):
    """cells one field's mirror writes: south Nz * Hy padded rows, bottom / top Hz padded planes each"""
    (nx, ny, nz), (hx, hy, hz) = size, halo
    sx, sy = nx + 2 * hx, ny + 2 * hy
    return (nz * hy * sx if sides & SOUTH else 0) + (hz * sx * sy if sides & BOTTOM else 0) + (hz * sx * sy if sides & TOP else 0)


def run_case(torch, osg, _lib, tlib, dev, size, h, tdt, specs):
    from tools import testlib
    halo = (h, h, h)
    ft, esz = (_lib.TPG_F64, 8) if tdt == torch.float64 else (_lib.TPG_F32, 4)
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo)
    nf, per = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition
    fs = []
    for k, (name, xl, yl, sides) in enumerate(specs):
        bcs = osg.FieldBoundaryConditions(west=per(), east=per(), south=nf() if sides & SOUTH else None,
                                          bottom=nf() if sides & BOTTOM else None, top=nf() if sides & TOP else None)
        f = osg.Field((osg.Face if xl else osg.Center, osg.Face if yl else osg.Center, osg.Center), grid, boundary_conditions=bcs)
        testlib.check(tlib.tpg_fill_synthetic(f.data.data_ptr(), 0xB0 + k, 12345.0, f.Nx, f.Ny, f.Nz, f.Hx, f.Hy, f.Hz, ft, None))
        fs.append(f)
    plan = osg.halo_fill_plan(fs)
    lib = _lib.lib()
    n = len(fs)
    pt = _lib.ptr_table([f.data for f in fs])
    st = (C.c_uint8 * n)(*[s[3] for s in specs])
    cells = sum(bounded_cells(size, halo, s[3]) for s in specs)
    nbytes = 2 * cells * esz
    src = torch.empty(cells, dtype=tdt, device=dev)
    dst = torch.empty(cells, dtype=tdt, device=dev)
    src.uniform_()
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache
    stream = _lib.current_stream_ptr(dev)

    def bounded():
        _lib.check(lib.tpg_fill_bounded_halos(pt, n, st, *size, *halo, ft, stream))

    def timed(fn):
        out = []
        for _ in range(REPS):
            flush.sum()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out[DROP:])

    plan(); bounded(); dst.copy_(src); torch.cuda.synchronize()              # warm: code objects, first-call queries
    t_fill, t_bounded, t_copy = timed(plan), timed(bounded), timed(lambda: dst.copy_(src))
    frac = lambda ms: nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
    out = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32", "fields": [s[0] for s in specs],
           "fill_ms": t_fill, "bounded_ms": t_bounded, "bounded_algorithmic_bytes": nbytes, "bounded_frac_of_hbm_peak": frac(t_bounded),
           "flat_copy_ms": t_copy, "flat_copy_frac_of_hbm_peak": frac(t_copy), "bounded_over_flat_copy_rate": t_copy / t_bounded,
           "bounded_share_of_fill": t_bounded / t_fill}
    del plan, fs, grid, src, dst, flush
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def config5(torch, osg, _lib, tlib, dev):
    size, h = (8640, 4320, 100), 5
    nx, ny, nz = size
    field_bytes = (nx + 2 * h) * (ny + 2 * h) * (nz + 2 * h) * 8
    free, total = torch.cuda.mem_get_info(dev)
    # per field: the field + its share of the flat-copy pair (2 x the cells the mirror writes); keep 40 % of what is free in reserve
    per_field = field_bytes + 2 * bounded_cells(size, (h, h, h), SOUTH | BOTTOM | TOP) * 8
    n = min(len(MODEL), int(0.6 * free // per_field))
    if n < 1:
        return {"skipped": f"one field needs {per_field / 1e9:.0f} GB, {free / 1e9:.0f} GB free"}
    torch.cuda.reset_peak_memory_stats(dev)
    out = run_case(torch, osg, _lib, tlib, dev, size, h, torch.float64, MODEL[:n])
    out["max_memory_allocated_GB"] = torch.cuda.max_memory_allocated(dev) / 1e9
    out["device_memory_GB"] = total / 1e9
    return out


def bench_bounded(torch, osg, _lib, tlib, dev, with_config5=True):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            out[f"headline_halo{h}_{tag}"] = run_case(torch, osg, _lib, tlib, dev, (3600, 1800, 75), h, tdt, MODEL)
    if with_config5:
        out["config5_halo5_f64"] = config5(torch, osg, _lib, tlib, dev)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call cold (after a 1 GiB read-only pass); fill_ms = stream-event "
                     "bracket around the HaloFillPlan call (merged horizontal fill + the bounded pass), bounded_ms = the same bracket around "
                     "the one-launch tpg_fill_bounded_halos call, flat_copy_ms = the same bracket around torch copy_ of "
                     "bounded_algorithmic_bytes / 2 bytes; fractions of 8 TB/s over algorithmic bytes (2 x cells written x sizeof(T))")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    from tools import testlib
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    print(json.dumps(bench_bounded(torch, osg, _lib, testlib.lib(), dev, with_config5="--no-config5" not in sys.argv)))


if __name__ == "__main__":
    main()
