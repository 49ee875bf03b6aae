"""bench_continuity.py -- w from continuity and the horizontal divergence (tpg_w_from_continuity).

Fields u, v, w, div at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell, on the grid's own metric arrays.
Per case this script times

  * hip_ms        -- tpg_w_from_continuity with w only: the one launch in a stream-event bracket;
  * hip_both_ms   -- the same launch writing w and div;
  * hip_fill_ms   -- the plan a host runs per step: the w-only launch and w's own halo fill;

and, beside them, what a reader needs to judge the pass:

  (a) floor_ms      the bytes the pass must move (u, v read, w written: (3 Nz + 1) interior planes, plus the three metric planes) x sizeof(T) / 8 TB/s;
  (b) flat_ms       a flat device pass of the same stream shape: torch.add(a, b, out=c) on contiguous tensors of the interior's size;
  (c) vorticity_ms  tpg_vertical_vorticity on the same u, v (the same three streams): THE YARDSTICK, alternating with hip_ms inside every
                    repetition, so that drift of the device lands on both alike;
  (d) torch_ms      the rule as a host of this library writes it without the call: the per-level loop of torch passes with temporaries;
  equals_torch      whether the HIP w and (d) agree bit for bit on the whole interior (NaNs by NaN-ness);
  variants_ms       with --variants PATH[,PATH...]: the w-only call through each of those builds of the library (the compile-time variants of
                    profiles/continuity/), alternating inside every repetition, and whether each leaves the product's bits.

Each figure: median of 10 after 2 dropped, every timed call after a 1 GiB read-only pass (the tensors are 2 - 4 GB each: no timed call finds
its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_continuity.py [--continuity-lib PATH] [--variants PATH,...] [--cases halo4_f64,...]   -> one JSON line.
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


def same_bits(torch, x, y):
    ints = torch.int64 if x.dtype == torch.float64 else torch.int32
    return bool(((x.contiguous().view(ints) == y.contiguous().view(ints)) | (x.isnan() & y.isnan())).all())


def run_case(torch, osg, _lib, dev, size, h, tdt, variants):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v])
    w, div = osg.ZFaceField(grid), osg.CenterField(grid)
    zeta = osg.Field((osg.Face, osg.Face, osg.Center), grid)
    plan = osg.continuity_plan(u, v, w)
    bare = osg.continuity_plan(u, v, w, fill_halos=False)
    both = osg.continuity_plan(u, v, w, div, fill_halos=False)
    vort = osg.vorticity_plan(u, v, zeta, fill_halos=False)

    dy, dx, az = grid.arrays["dy_fc"], grid.arrays["dx_cf"], grid.arrays["az_cc"]
    dz = [float(d) for d in osg.z_center_spacings(grid, tdt)]     # exact values of the type
    rows, cols = slice(hy, hy + ny), slice(hx, hx + nx)
    az_in = az[rows, cols]
    inner = lambda f, levels: f.data[hz:hz + levels, rows, cols]

    def composition():
        """the rule, level by level: every line a full-plane torch pass with a temporary"""
        out = torch.empty((nz + 1, ny, nx), dtype=tdt, device=dev)
        out[0] = 0
        for k in range(nz):
            d = dz[k]
            fx = (dy[rows, hx:hx + nx + 1] * d) * u.data[hz + k, rows, hx:hx + nx + 1]
            fy = (dx[hy:hy + ny + 1, cols] * d) * v.data[hz + k, hy:hy + ny + 1, cols]
            dv = (1 / (az_in * d)) * ((fx[:, 1:] - fx[:, :-1]) + (fy[1:] - fy[:-1]))
            out[k + 1] = out[k] - d * dv
        return out

    cells = nx * ny * nz
    nbytes = ((3 * nz + 1) + 3) * nx * ny * esz
    flat = [torch.empty(cells, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen) for _ in range(2)] + [torch.empty(cells, dtype=tdt, device=dev)]
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

    plan(); bare(); both(); vort(); torch.cuda.synchronize()               # warm: code objects, first-call queries
    ref = composition()
    equal = same_bits(torch, inner(w, nz + 1), ref)
    del ref
    pair = alternating({"hip_ms": bare, "vorticity_ms": vort})
    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32", "bytes": nbytes,
           "hip_ms": pair["hip_ms"], "vorticity_ms": pair["vorticity_ms"], "hip_both_ms": timed(both), "hip_fill_ms": timed(plan),
           "floor_ms": nbytes / (HBM_PEAK_GBPS * 1e9) * 1e3, "flat_ms": timed(lambda: torch.add(flat[0], flat[1], out=flat[2])),
           "torch_ms": timed(composition), "equals_torch": equal}
    res["over_vorticity_time"] = res["hip_ms"] / res["vorticity_ms"]
    res["frac_of_hbm_peak"] = res["floor_ms"] / res["hip_ms"]
    res["over_flat_time"] = res["hip_ms"] / res["flat_ms"]
    res["torch_over_hip_time"] = res["torch_ms"] / res["hip_ms"]
    if variants:
        # the same w-only call through other builds of the library: compile-time variants, alternating inside every repetition
        _, args = bare._call
        stream = _lib.current_stream_ptr(dev)
        want = inner(w, nz + 1).clone()
        fns, same = {}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.CONTINUITY_SIGNATURES)
            call = (lambda hd: lambda: _lib.check_continuity(hd.tpg_w_from_continuity(*args, stream)))(handle)
            w.data.zero_()
            call()
            same[name] = same_bits(torch, inner(w, nz + 1), want)
            fns[name] = call
        res["variants_ms"] = alternating(fns)
        res["variants_same_bits"] = same
        del want
    del plan, bare, both, vort, u, v, w, div, zeta, flat, flush, grid, dx, dy, az, az_in
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_continuity(torch, osg, _lib, dev, variants=(), cases=None):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            name = f"halo{h}_{tag}"
            if cases is None or name in cases:
                out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, variants)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call "
                     "with w only (hip_ms), with w and div (hip_both_ms) or the plan with w's halo fill (hip_fill_ms); floor = ((3 Nz + 1) "
                     "interior planes + 3 metric planes) x sizeof(T) / 8 TB/s; flat = torch.add(a, b, out=c) on contiguous tensors of the "
                     "interior's size; vorticity = tpg_vertical_vorticity on the same u, v, alternating with hip_ms inside every repetition; "
                     "torch = the rule as the per-level loop of torch passes with temporaries; variants_ms = the w-only call through other "
                     "builds of the library, alternating inside every repetition")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--continuity-lib"):
        _lib.CONTINUITY_LIB_PATH = os.path.abspath(arg("--continuity-lib"))
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_continuity(torch, osg, _lib, dev, variants, cases)
    out["continuity_library"] = os.path.relpath(_lib.CONTINUITY_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
