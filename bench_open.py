"""bench_open.py -- the Open (impenetrable) south / bottom / top face write (tpg_fill_open_faces).

Fields u, v, w, T, S at 3600 x 1800 x 75 with a model's default sides: v south impenetrable, w bottom / top impenetrable, every Center side
no-flux.  Before the horizontal fill the library writes the boundary faces of v and w: one launch per geometry group that has an Open side
(v with the Nz-level fields, w alone with its Nz + 1 levels).  This script times, per case:

  * fill_ms  -- the whole five-field fill: a stream-event bracket around the HaloFillPlan call (every launch it makes);
  * open_ms  -- the tpg_fill_open_faces calls of the plan alone, in one stream-event bracket (two launches);
  * open_algorithmic_bytes = cells written x sizeof(T) + condition cells read x sizeof(T), and its fraction of 8 TB/s;
  * flat_ms  -- beside it, the same number of bytes moved flat and timed the same way: a device fill (torch zero_) of the written bytes
                in the scalar cases, a device copy (torch copy_) of as many elements as are written in the array case.

Cases: halo 4 and (5, 5, 5), Float64 and Float32, impenetrable sides; one more with array conditions on all three sides (halo 5,
Float64).  Each figure: median of 10 after 2 dropped, cold (after a 1 GiB read-only pass).
Runnable alone:  python bench_open.py [--product-lib PATH]   -> one JSON line  (PATH: another build of the product library, e.g. one with
-DTPG_OPEN_NT=1, for the A/B of the store hint).
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
REPS, DROP = 12, 2
SIZE = (3600, 1800, 75)


def _open_calls(plan):
    return [(fn, args) for _, calls, _ in plan._steps for fn, args, *_ in calls if fn.__name__ == "tpg_fill_open_faces"]


def run_case(torch, osg, _lib, tlib, dev, size, h, tdt, arrays):
    from tools import testlib
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    sx, sy = nx + 2 * hx, ny + 2 * hy
    esz = 8 if tdt == torch.float64 else 4
    ft = _lib.ft_of(tdt)
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo)
    nf, per, O = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition, osg.OpenBoundaryCondition
    cond = lambda rows: torch.empty(rows, sx, dtype=tdt, device=dev).uniform_(-1e-3, 1e-3)
    v_south, w_bottom, w_top = (cond(nz), cond(sy), cond(sy)) if arrays else (None, None, None)
    Ce, Fa = osg.Center, osg.Face
    specs = [("u", (Fa, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())), ("v", (Ce, Fa, Ce), dict(south=O(v_south), bottom=nf(), top=nf())),
             ("w", (Ce, Ce, Fa), dict(south=nf(), bottom=O(w_bottom), top=O(w_top))), ("T", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())),
             ("S", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf()))]
    fs = []
    for k, (name, loc, sides) in enumerate(specs):
        f = osg.Field(loc, grid, name=name, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))
        testlib.check(tlib.tpg_fill_synthetic(f.data.data_ptr(), 0xD0 + k, 12345.0, f.Nx, f.Ny, f.Nz, f.Hx, f.Hy, f.Hz, ft, None))
        fs.append(f)
    plan = osg.halo_fill_plan(fs)
    open_calls = _open_calls(plan)
    assert len(open_calls) == 2 and all(calls[0][0].__name__ == "tpg_fill_open_faces" for _, calls, _ in plan._steps)
    cells = nz * sx + 2 * ny * sx                                      # v: row 1 of Nz levels; w: rows 1..Ny of its two face planes
    nbytes = cells * esz * (2 if arrays else 1)
    dst = torch.empty(cells, dtype=tdt, device=dev)
    src = torch.empty(cells, dtype=tdt, device=dev).uniform_() if arrays else None
    flat = (lambda: dst.copy_(src)) if arrays else (lambda: dst.zero_())
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache
    stream = _lib.current_stream_ptr(dev)

    def call(which):
        def go():
            for fn, args in which:
                _lib.check(fn(*args, stream))
        return go

    def timed(fn):
        out = []
        for _ in range(REPS):
            flush.sum()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out[DROP:])

    plan(); call(open_calls)(); flat(); torch.cuda.synchronize()           # warm: code objects, first-call queries
    t_fill, t_open, t_flat = timed(plan), timed(call(open_calls)), timed(flat)
    t_v, t_w = timed(call(open_calls[:1])), timed(call(open_calls[1:]))
    frac = lambda ms: nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
    out = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32", "fields": [s[0] for s in specs],
           "conditions": "arrays" if arrays else "impenetrable", "fill_ms": t_fill, "open_ms": t_open, "open_v_ms": t_v, "open_w_ms": t_w,
           "open_algorithmic_bytes": nbytes, "open_frac_of_hbm_peak": frac(t_open), "flat": "copy_" if arrays else "zero_",
           "flat_ms": t_flat, "flat_frac_of_hbm_peak": frac(t_flat), "open_over_flat_time": t_open / t_flat, "open_share_of_fill": t_open / t_fill}
    del plan, fs, grid, src, dst, flush, v_south, w_bottom, w_top
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def bench_open(torch, osg, _lib, tlib, dev):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            out[f"model_halo{h}_{tag}"] = run_case(torch, osg, _lib, tlib, dev, SIZE, h, tdt, False)
    out["model_halo5_f64_arrays"] = run_case(torch, osg, _lib, tlib, dev, SIZE, 5, torch.float64, True)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call cold (after a 1 GiB read-only pass); fill_ms = stream-event "
                     "bracket around the HaloFillPlan call of (u, v, w, T, S): per geometry group the Open launch, the merged horizontal "
                     "fill and the no-flux mirror; open_ms = the same bracket around the two tpg_fill_open_faces calls (v's group, then "
                     "w's), open_v_ms / open_w_ms each alone; flat_ms = the same bracket around torch zero_ of the written bytes (scalar "
                     "cases) or torch copy_ of as many elements (array case); fractions of 8 TB/s over algorithmic bytes (cells written x "
                     "sizeof(T), plus as many condition cells read in the array case)")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    if "--product-lib" in sys.argv:
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--product-lib") + 1])
    from tools import testlib
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_open(torch, osg, _lib, testlib.lib(), dev)
    out["product_library"] = os.path.relpath(_lib.LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
