"""bench_free_surface.py -- the split-explicit free-surface sub-step (tpg_free_surface_substep) and the sub-cycle plan.

A free surface of 30 sub-steps on 3600 x 1800, halo 4 and (5, 5, 5), Float64 and Float32: its 2-D fields live on the extended-halo grid
(Hy2 = 31), random values in every cell, averaging on.  Per case this script times

  * substep_ms      -- tpg_free_surface_substep, the one launch in a stream-event bracket;
  * copy_ms         -- THE YARDSTICK: a flat device copy (dst.copy_(src) on contiguous tensors) that moves the bytes the sub-step must move,
                       alternating with substep_ms inside every repetition, so that drift of the device lands on both alike.  Those bytes
                       are `arrays_read` (13 interior planes: eta, U, V, GU, GV, the five metrics, the three averages) and `arrays_written`
                       (6: eta, U, V of the other set and the three averages): 19 planes, so the copy reads 9.5 and writes 9.5;
  * substep_floor_ms   those bytes / 8 TB/s;
  * torch_ms        -- the same sub-step as a host of this library writes it without the call: a composition of elementwise torch passes on
                       slices; substep_equals_torch: whether the two leave identical bits on the whole interiors (NaNs by NaN-ness),
                       checked before timing;
  * fill_ms         -- one HaloFillPlan of (eta, U, V), what follows every sub-step;
  * plan_eager_ms / plan_graph_ms   the 30-sub-step plan (sub-step + fill, x 30, the averages zeroed first and filled last) called eagerly and
                       replayed as ONE graph; per_substep = / 30;
  * variants_ms     -- with --variants PATH[,PATH...]: the call through each of those builds of the library (the compile-time variants of
                       profiles/free_surface/), alternating inside every repetition, and whether each leaves the product's bits.

Each figure: median of 10 after 2 dropped, every timed call after a 1 GiB read-only pass.
Runnable alone:  python bench_free_surface.py [--variants PATH,...] [--cases halo4_f64,...]   -> one JSON line.
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
SUBSTEPS = 30
DTAU = 1.0
ARRAYS_READ = ["eta_in", "U_in", "V_in", "GU", "GV", "dy_fc", "dx_cf", "az_cc", "dx_fc", "dy_cf", "eta_bar", "U_bar", "V_bar"]
ARRAYS_WRITTEN = ["eta_out", "U_out", "V_out", "eta_bar", "U_bar", "V_bar"]


def same_bits(torch, x, y):
    ints = torch.int64 if x.dtype == torch.float64 else torch.int32
    return bool(((x.contiguous().view(ints) == y.contiguous().view(ints)) | (x.isnan() & y.isnan())).all())


def run_case(torch, osg, _lib, dev, size, h, tdt, variants):
    from orthogonalsphericalshellgrids.jl_amd.free_surface import _Substep
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    fs = osg.SplitExplicitFreeSurface(grid, substeps=SUBSTEPS)
    ext = fs.extended_grid
    hy2 = ext.Hy
    gen = torch.Generator(device=dev).manual_seed(7)
    for f in (*fs.state, *fs.twins, *fs.averages, fs.GU, fs.GV):
        f.data.uniform_(-1, 1, generator=gen)
    fill = osg.halo_fill_plan(list(fs.state))
    fill()
    weight = fs.weights[0]
    g = fs.gravitational_acceleration
    step = _Substep(fs.twins, fs.state, (fs.GU, fs.GV), fs.averages, DTAU, g, weight, grid, "bench_free_surface")
    plan = osg.split_explicit_subcycle_plan(fs, DTAU)

    rows, cols = slice(hy2, hy2 + ny), slice(hx, hx + nx)
    east, north = slice(hx + 1, hx + nx + 1), slice(hy2 + 1, hy2 + ny + 1)
    m = {k: ext.arrays[k] for k in ("dy_fc", "dx_cf", "az_cc", "dx_fc", "dy_cf")}
    gH = torch.tensor(g, dtype=tdt, device=dev) * osg.column_depth_table(ext, tdt)[0].to(tdt).to(dev)    # a 0-dim tensor of the type: g * H, once

    def torch_substep(src, dst, bars):
        """the rule as elementwise torch passes on slices, each with a temporary: what a host writes without the call"""
        eta, U, V = (f.data[0] for f in src)
        fe, fw = m["dy_fc"][rows, east] * U[rows, east], m["dy_fc"][rows, cols] * U[rows, cols]
        fn, fs_ = m["dx_cf"][north, cols] * V[north, cols], m["dx_cf"][rows, cols] * V[rows, cols]
        d = ((fe - fw) + (fn - fs_)) / m["az_cc"][rows, cols]
        etap = eta[rows, cols] - DTAU * d
        px = (etap - torch.roll(etap, 1, dims=1)) / m["dx_fc"][rows, cols]
        Up = U[rows, cols] + DTAU * (fs.GU.data[0][rows, cols] - gH * px)
        py = (etap[1:] - etap[:-1]) / m["dy_cf"][rows, cols][1:]
        Vp = V[rows, cols].clone()
        Vp[1:] = V[rows, cols][1:] + DTAU * (fs.GV.data[0][rows, cols][1:] - gH * py)
        for f, b, x in zip(dst, bars, (etap, Up, Vp)):
            f.data[0][rows, cols] = x
            b.data[0][rows, cols] += weight * x

    plane = nx * ny
    half = (len(ARRAYS_READ) + len(ARRAYS_WRITTEN)) * plane // 2
    flat = [torch.empty(half, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(half, dtype=tdt, device=dev)]
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def once(fn):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn):
        return statistics.median([once(fn) for _ in range(REPS)][DROP:])

    def alternating(fns):
        """{name: median}: the calls alternate inside every repetition"""
        samples = {name: [] for name in fns}
        for _ in range(REPS):
            for name, fn in fns.items():
                samples[name].append(once(fn))
        return {name: statistics.median(s[DROP:]) for name, s in samples.items()}

    # the same bits: the call and the composition from one state into two sets of outputs and averages
    new = lambda f: osg.Field(f.loc, ext)
    tw, tb = [new(f) for f in fs.state], [new(f) for f in fs.averages]
    for a, b in zip(tb, fs.averages):
        a.data.copy_(b.data)
    step()
    torch_substep(fs.state, tw, tb)
    torch.cuda.synchronize()
    inner = lambda f: f.data[0][rows, cols]
    equal = all(same_bits(torch, inner(a), inner(b)) for a, b in zip((*fs.twins, *fs.averages), (*tw, *tb)))

    pair = alternating({"substep_ms": step, "copy_ms": lambda: flat[1].copy_(flat[0])})
    nbytes = (len(ARRAYS_READ) + len(ARRAYS_WRITTEN)) * plane * esz
    res = {"size": [nx, ny], "halo": list(halo), "Hy2": hy2, "substeps": SUBSTEPS, "eltype": "Float64" if esz == 8 else "Float32",
           "arrays_read": ARRAYS_READ, "arrays_written": ARRAYS_WRITTEN, "substep_bytes": nbytes, **pair,
           "substep_floor_ms": nbytes / (HBM_PEAK_GBPS * 1e9) * 1e3, "torch_ms": timed(lambda: torch_substep(fs.state, tw, tb)),
           "substep_equals_torch": equal, "fill_ms": timed(fill)}
    res["substep_over_copy_time"] = res["substep_ms"] / res["copy_ms"]
    res["substep_frac_of_hbm_peak"] = res["substep_floor_ms"] / res["substep_ms"]
    res["torch_over_substep_time"] = res["torch_ms"] / res["substep_ms"]
    if variants:
        # the same call through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        start = [f.data.clone() for f in fs.averages]

        def from_start(fn):
            for f, t in zip(fs.averages, start):
                f.data.copy_(t)
            for f in fs.twins:
                f.data.zero_()
            fn()
            return [inner(f).clone() for f in (*fs.twins, *fs.averages)]

        want = from_start(step)
        fv, same = {}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.FREE_SURFACE_SIGNATURES)
            fv[name] = (lambda hd: lambda: _lib.check_free_surface(hd.tpg_free_surface_substep(*step._args, stream)))(handle)
            same[name] = all(same_bits(torch, x, w) for x, w in zip(from_start(fv[name]), want))
        res["variants_ms"] = alternating({"product": step, **fv})
        res["variants_same_bits"] = same
        del want, start
    # the whole sub-cycle: eagerly, and as one replayed graph
    plan()
    torch.cuda.synchronize()
    res["plan_eager_ms"] = timed(plan)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        plan()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    res["plan_graph_ms"] = timed(graph.replay)
    res["plan_eager_per_substep_ms"] = res["plan_eager_ms"] / SUBSTEPS
    res["plan_graph_per_substep_ms"] = res["plan_graph_ms"] / SUBSTEPS
    del graph, plan, step, fill, fs, tw, tb, flat, flush, grid, ext, m
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_free_surface(torch, osg, _lib, dev, variants=(), cases=None):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            name = f"halo{h}_{tag}"
            if cases is None or name in cases:
                out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, variants)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call "
                     "(substep_ms), the plan's 30 sub-steps and fills (plan_eager_ms) or one graph replay of them (plan_graph_ms); copy = "
                     "dst.copy_(src) on contiguous tensors of 9.5 interior planes (the 19 planes the sub-step reads and writes), alternating "
                     "with substep_ms inside every repetition; floor = those bytes / 8 TB/s; torch = the rule as elementwise torch passes on "
                     "slices; variants = the call through other builds of the library, alternating")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_free_surface(torch, osg, _lib, dev, variants, cases)
    out["free_surface_library"] = os.path.relpath(_lib.FREE_SURFACE_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
