"""bench_value_gradient.py -- the Value / Gradient south / bottom / top halo fill (tpg_fill_value_gradient_halos).

Fields at 3600 x 1800 x 75: T and S with a Value top (a scalar surface value) and a Gradient bottom (a scalar stratification), and c with
a tensor-valued Value top and a Gradient south.  After the horizontal fill (zipper -> periodic x, one merged launch) the library writes the
first halo point of those sides in two more launches: the south pass, then the bottom / top pass.  This script times, per case:

  * fill_ms  -- the whole fill: a stream-event bracket around the HaloFillPlan call (every launch it makes);
  * vg_ms    -- the two Value / Gradient calls, south then bottom / top, in one stream-event bracket (two launches); south_ms and z_ms
                each alone;
  * vg_algorithmic_bytes = 2 x cells written x sizeof(T) + the condition arrays read + one dy_cf row, and its fraction of 8 TB/s;
  * copy_ms  -- beside it, a flat device copy (torch copy_) of the same number of bytes, timed the same way;
  * z_all_gradient_ms -- the bottom / top pass of the same fields with every Value side made a Gradient side (same bytes, no division):
                the cost of the Value form's per-element division.

Cases: halo 4 and (5, 5, 5), Float64 and Float32.  Each figure: median of 10 after 2 dropped, cold (after a 1 GiB read-only pass).
Runnable alone:  python bench_value_gradient.py   -> one JSON line.
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


def _vg_calls(plan):
    (_, calls, _), = plan._steps
    return [(fn, args) for fn, args, *_ in calls if fn.__name__ == "tpg_fill_value_gradient_halos"]


def run_case(torch, osg, _lib, tlib, dev, size, h, tdt):
    from tools import testlib
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    sx, sy = nx + 2 * hx, ny + 2 * hy
    esz = 8 if tdt == torch.float64 else 4
    ft = _lib.ft_of(tdt)
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo)
    V, G, per = osg.ValueBoundaryCondition, osg.GradientBoundaryCondition, osg.PeriodicBoundaryCondition
    c_top = torch.empty(sy, sx, dtype=tdt, device=dev).uniform_(0, 1)
    specs = [("T", dict(top=V(20.0), bottom=G(1e-4))), ("S", dict(top=V(35.0), bottom=G(-2e-5))), ("c", dict(top=V(c_top), south=G(1e-3)))]
    fs = []
    for k, (name, sides) in enumerate(specs):
        f = osg.CenterField(grid, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))
        testlib.check(tlib.tpg_fill_synthetic(f.data.data_ptr(), 0xC0 + k, 12345.0, f.Nx, f.Ny, f.Nz, f.Hx, f.Hy, f.Hz, ft, None))
        fs.append(f)
    plan = osg.halo_fill_plan(fs)
    vg_calls = _vg_calls(plan)
    assert [a[2] for _, a in vg_calls] == [_lib.TPG_SIDE_SOUTH, _lib.TPG_SIDE_BOTTOM | _lib.TPG_SIDE_TOP]
    grad = lambda bc: G(bc.condition) if osg.is_value(bc) else bc
    twins = [osg.CenterField(grid, data=f.data, boundary_conditions=osg.FieldBoundaryConditions(
        west=per(), east=per(), **{k: grad(b) for k, b in sides.items()})) for f, (_, sides) in zip(fs, specs)]
    z_grad = _vg_calls(osg.halo_fill_plan(twins))[1:]
    cells = 2 * sx * sy + 2 * sx * sy + (sx * sy + nz * sx)          # T, S: bottom + top planes; c: top plane + south rows
    cond_reads = sx * sy + sx                                          # c's top condition array + one dy_cf row
    nbytes = (2 * cells + cond_reads) * esz
    src = torch.empty(nbytes // 2 // esz, dtype=tdt, device=dev).uniform_()
    dst = torch.empty_like(src)
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

    plan(); call(vg_calls)(); dst.copy_(src); torch.cuda.synchronize()      # warm: code objects, first-call queries
    t_fill, t_vg = timed(plan), timed(call(vg_calls))
    t_south, t_z = timed(call(vg_calls[:1])), timed(call(vg_calls[1:]))
    t_zg = timed(call(z_grad))
    t_copy = timed(lambda: dst.copy_(src))
    frac = lambda ms: nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS
    out = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32", "fields": [s[0] for s in specs],
           "fill_ms": t_fill, "vg_ms": t_vg, "south_ms": t_south, "z_ms": t_z, "z_all_gradient_ms": t_zg, "vg_algorithmic_bytes": nbytes,
           "vg_frac_of_hbm_peak": frac(t_vg), "flat_copy_ms": t_copy, "flat_copy_frac_of_hbm_peak": frac(t_copy),
           "vg_over_flat_copy_time": t_vg / t_copy, "vg_share_of_fill": t_vg / t_fill}
    del plan, fs, twins, grid, src, dst, flush, c_top
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def bench_value_gradient(torch, osg, _lib, tlib, dev):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            out[f"headline_halo{h}_{tag}"] = run_case(torch, osg, _lib, tlib, dev, SIZE, h, tdt)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call cold (after a 1 GiB read-only pass); fill_ms = stream-event "
                     "bracket around the HaloFillPlan call (merged horizontal fill + the two Value / Gradient launches), vg_ms = the same "
                     "bracket around the two tpg_fill_value_gradient_halos calls (south, then bottom / top), south_ms / z_ms each alone, "
                     "z_all_gradient_ms = z_ms with every Value side made a Gradient side (same bytes, no division), "
                     "flat_copy_ms = the same bracket around torch copy_ of vg_algorithmic_bytes / 2 bytes; fractions of 8 TB/s over "
                     "algorithmic bytes (2 x cells written x sizeof(T) + condition array + one dy_cf row)")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    from tools import testlib
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    print(json.dumps(bench_value_gradient(torch, osg, _lib, testlib.lib(), dev)))


if __name__ == "__main__":
    main()
