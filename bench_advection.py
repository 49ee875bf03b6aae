"""bench_advection.py -- the flux-form advection tendency of the tracers (tpg_tracer_advection_tendency).

Fields at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell, with n = 1, 2 and 4 tracers in a call.
Per case and n this script times, each as the one launch in a stream-event bracket around the C call,

  * call{n}_ms      -- tpg_tracer_advection_tendency on n tracers: u, v, w and n tracers read, n tendencies written: (3 + 2n) 3-D streams,
                       w one level longer;

and, beside them, what a reader needs to judge the pass:

  (a) floor{n}_ms   the bytes the call must move x sizeof(T) / 8 TB/s;
  (b) copy{n}_ms    a flat device copy of the same bytes (dst.copy_(src) on contiguous tensors, half the bytes read and half written): THE
                    YARDSTICK of the project's streams, alternating with the call inside every repetition, so that drift of the device lands
                    on both alike;
  (c) torch1_ms     the parent commit's way of doing the call's work for one tracer: the same rule as torch elementwise passes on slices of
                    the parents (every product, mean and difference a pass and a temporary of its own), alternating with call1_ms;
  equals_torch      whether HIP and (c) agree bit for bit on the whole parent of G (NaNs by NaN-ness), checked before timing;
  variants          with --variants PATH[,PATH...]: the 1-, 2- and 4-tracer calls through each of those builds of the library (the
                    compile-time variants of profiles/advection/), alternating inside every repetition, with the range of the samples, and
                    whether each leaves the product's bits.

Each figure: median of 10 after 2 dropped (`*_range`: the least and the greatest of the 10), every timed call after a 1 GiB read-only pass
(the tensors are 2 - 4 GB each: no timed call finds its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_advection.py [--advection-lib PATH] [--variants PATH,...] [--cases halo4_f64,...] [--no-torch]   -> one JSON line.
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPS, DROP = 12, 2
SIZE = (NX, NY, NZ)
TRACERS = (1, 2, 4)


def same_bits(torch, x, y):
    ints = torch.int64 if x.dtype == torch.float64 else torch.int32
    return bool(((x.contiguous().view(ints) == y.contiguous().view(ints)) | (x.isnan() & y.isnan())).all())


def run_case(torch, osg, _lib, dev, size, h, tdt, variants, with_torch):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, G = ([osg.CenterField(grid) for _ in range(max(TRACERS))] for _ in range(2))
    for f in (u, v, w, *c):
        f.data.uniform_(-1, 1, generator=gen)
    plans = {n: osg.tracer_advection_plan(c[:n], u, v, w, G[:n]) for n in TRACERS}

    cells = nx * ny * nz
    face_cells = nx * ny * (nz + 1)
    elems = {n: (2 + 2 * n) * cells + face_cells for n in TRACERS}                        # u, v, n tracers, n tendencies; w one level longer
    top = (max(elems.values()) + 1) // 2
    flat = [torch.empty(top, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(top, dtype=tdt, device=dev)]
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def copy_of(n):
        half = elems[n] // 2
        return lambda: flat[1][:half].copy_(flat[0][:half])

    def once(fn):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def alternating(fns):
        """({name: median}, {name: [least, greatest]}): the calls alternate inside every repetition"""
        samples = {name: [] for name in fns}
        for _ in range(REPS):
            for name, fn in fns.items():
                samples[name].append(once(fn))
        return ({name: statistics.median(s[DROP:]) for name, s in samples.items()},
                {name + "_range": [min(s[DROP:]), max(s[DROP:])] for name, s in samples.items()})

    g = getattr(grid, "underlying_grid", grid)
    dy, dx, az = (g.arrays[k] for k in ("dy_fc", "dx_cf", "az_cc"))
    dz = osg.z_center_spacings(grid, tdt).to(tdt).to(dev)[:, None, None]
    zs, ys, xs = slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx)
    out_t = osg.CenterField(grid)
    one = torch.ones((), dtype=tdt, device=dev)

    def torch_tendency(cq, out):
        """the rule as a host writes it in torch: every line full 3-D elementwise passes, each product a temporary of its own"""
        cd = cq.data
        Mx = (dy[None, ys, hx:hx + nx + 1] * dz) * u.data[zs, ys, hx:hx + nx + 1]
        Fx = Mx * (0.5 * (cd[zs, ys, hx - 1:hx + nx] + cd[zs, ys, hx:hx + nx + 1]))
        del Mx
        acc = Fx[:, :, 1:] - Fx[:, :, :-1]
        del Fx
        My = (dx[None, hy:hy + ny + 1, xs] * dz) * v.data[zs, hy:hy + ny + 1, xs]
        Fy = My * (0.5 * (cd[zs, hy - 1:hy + ny, xs] + cd[zs, hy:hy + ny + 1, xs]))
        del My
        acc = acc + (Fy[:, 1:, :] - Fy[:, :-1, :])
        del Fy
        Mz = az[None, ys, xs] * w.data[hz:hz + nz + 1, ys, xs]
        Fz = Mz * (0.5 * (cd[hz - 1:hz + nz, ys, xs] + cd[hz:hz + nz + 1, ys, xs]))
        del Mz
        acc = acc + (Fz[1:] - Fz[:-1])
        del Fz
        V = az[None, ys, xs] * dz
        out.data[zs, ys, xs] = -(torch.div(one, V) * acc)                 # a division, not a reciprocal approximation

    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    for n in TRACERS:
        plans[n]()
    torch.cuda.synchronize()
    if with_torch:
        out_t.data.copy_(G[0].data)                                 # the halo cells: as the call left them (untouched)
        out_t.data[zs, ys, xs] = 0
        torch_tendency(c[0], out_t)
        torch.cuda.synchronize()
        res["equals_torch"] = same_bits(torch, G[0].data, out_t.data)
    floor = lambda b: b / (HBM_PEAK_GBPS * 1e9) * 1e3
    for n in TRACERS:
        fns = {f"call{n}_ms": plans[n], f"copy{n}_ms": copy_of(n)}
        if with_torch and n == 1:
            fns["torch1_ms"] = lambda: torch_tendency(c[0], out_t)
        med, rng = alternating(fns)
        res.update(med)
        res.update(rng)
        res[f"bytes{n}"] = elems[n] * esz
        res[f"floor{n}_ms"] = floor(elems[n] * esz)
        res[f"call{n}_over_copy_time"] = res[f"call{n}_ms"] / res[f"copy{n}_ms"]
        res[f"call{n}_frac_of_hbm_peak"] = res[f"floor{n}_ms"] / res[f"call{n}_ms"]
    if with_torch:
        res["torch_over_call1_time"] = res["torch1_ms"] / res["call1_ms"]
    res["call2_over_twice_call1"] = res["call2_ms"] / (2 * res["call1_ms"])
    res["call4_over_four_call1"] = res["call4_ms"] / (4 * res["call1_ms"])
    if variants:
        # the same calls through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        args = {n: plans[n]._call[1] for n in TRACERS}
        want = [f.data.clone() for f in G]
        fns, same = {f"product_{n}": plans[n] for n in TRACERS}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.ADVECTION_SIGNATURES)
            for n in TRACERS:
                fns[f"{name}_{n}"] = (lambda hd, a: lambda: _lib.check_advection(hd.tpg_tracer_advection_tendency(*a, stream)))(handle, args[n])
            for f in G:
                f.data.zero_()
            fns[f"{name}_{max(TRACERS)}"]()
            same[name] = all(same_bits(torch, f.data, t) for f, t in zip(G, want))
        med, rng = alternating(fns)
        res["variants_ms"] = med
        res["variants_range_ms"] = rng
        res["variants_same_bits"] = same
        del want
    del plans, u, v, w, c, G, out_t, flat, flush, grid
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_advection(torch, osg, _lib, dev, variants=(), cases=None, with_torch=True):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            name = f"halo{h}_{tag}"
            if cases is None or name in cases:
                out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, variants, with_torch)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call; "
                     "floors = the bytes each call must move ((3 + 2n) streams, w one level longer) x sizeof(T) / 8 TB/s; copy = dst.copy_(src) on "
                     "contiguous tensors of half those bytes, alternating with the call inside every repetition; torch = the rule as torch "
                     "elementwise passes on slices of the parents, alternating too; variants = the 1-, 2- and 4-tracer calls through other builds "
                     "of the library, alternating; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--advection-lib"):
        _lib.ADVECTION_LIB_PATH = os.path.abspath(arg("--advection-lib"))
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_advection(torch, osg, _lib, dev, variants, cases, "--no-torch" not in sys.argv)
    out["advection_library"] = os.path.relpath(_lib.ADVECTION_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
