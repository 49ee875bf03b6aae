"""bench_weno_xyz.py -- the tracer tendency of `WENO()`: WENO5 in x, y and z, walls in z (tpg_weno_xyz_tracer_advection_tendency).

Fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in every cell, one tracer.  Per case this script times, each as the
one launch in a stream-event bracket around the C call,

  * call_ms         -- tpg_weno_xyz_tracer_advection_tendency: u, v, w and the tracer read, the tendency written: five 3-D streams, w one
                       level longer;

and, beside it, what a reader needs to judge the pass:

  (1) weno_ms       tpg_weno_tracer_advection_tendency on the same inputs: the same kernel family with the centred mean in z (2.5 face
                    evaluations per node against this call's 3.5);
  (2) copy_ms       a flat device copy of the same bytes (dst.copy_(src) on contiguous tensors, half the bytes read and half written);
  (3) torch_ms      the rule as torch elementwise passes on slices of the parents (every product, select and difference a pass and a
                    temporary of its own; the z-faces of a class in one pass each); THE CONDITION: call_ms is below it with disjoint ranges;
  floor_ms          the bytes the call must move x sizeof(T) / 8 TB/s;
  equals_torch      whether HIP and (3) agree bit for bit on the whole parent of G (NaNs by NaN-ness), checked before timing;
  variants          with --variants PATH[,PATH...]: the call through each of those builds of the library (the compile-time variants of
                    profiles/weno_xyz/), alternating inside every repetition, with the range of the samples, and whether each leaves the
                    product's bits.

All of (1), (2), (3) and the call alternate inside every repetition, so that drift of the device lands on all alike.  Each figure: median of
5 after 2 dropped (`*_range`: the least and the greatest of the 5), every timed call after a 1 GiB read-only pass (the tensors are 2 - 4 GB
each: no timed call finds its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_weno_xyz.py [--weno-xyz-lib PATH] [--variants PATH,...] [--cases f64,f32] [--no-torch] [--calls-only N]  -> one JSON line.
`--calls-only N` issues the call N times on the first case and nothing else: the run a counter collection wraps.
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT
from bench_weno import same_bits, torch_rule

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPS, DROP = 7, 2
SIZE = (NX, NY, NZ)
HALO = 4


def torch_rule3(torch, tdt, dev):
    """R3 of include/tripolar_hip_weno_xyz.h as torch passes, the constants computed in the type"""
    t = lambda x: torch.tensor(x, dtype=tdt, device=dev)
    k23, k13, eps = t(2) / t(3), t(1) / t(3), t(1e-8)

    def face_value3(q0, q1, q2):
        p1 = 1.5 * q1 - 0.5 * q0
        p0 = 0.5 * (q1 + q2)
        e1 = q1 - q0
        b1 = e1 * e1
        e0 = q2 - q1
        b0 = e0 * e0
        tau = (b0 - b1).abs()
        r0, r1 = tau / (b0 + eps), tau / (b1 + eps)
        a0, a1 = k23 * (1 + r0 * r0), k13 * (1 + r1 * r1)
        return (a0 * p0 + a1 * p1) / (a0 + a1)

    return face_value3


def run_case(torch, osg, _lib, dev, size, tdt, variants, with_torch, calls_only=0):
    halo = (HALO, HALO, HALO)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, G = osg.CenterField(grid), osg.CenterField(grid)
    for f in (u, v, w, c):
        f.data.uniform_(-1, 1, generator=gen)
    plan = osg.weno_xyz_tracer_advection_plan([c], u, v, w, [G])
    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    if calls_only:
        for _ in range(calls_only):
            plan()
        torch.cuda.synchronize()
        res["calls"] = calls_only
        return res
    weno = osg.weno_tracer_advection_plan([c], u, v, w, [G])

    elems = 4 * nx * ny * nz + nx * ny * (nz + 1)                           # u, v, the tracer, the tendency; w one level longer
    flat = [torch.empty((elems + 1) // 2, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty((elems + 1) // 2, dtype=tdt, device=dev)]
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

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
    upwind, face3 = torch_rule(torch, tdt, dev), torch_rule3(torch, tdt, dev)

    def torch_tendency(cq, out):
        """the rule as a host writes it in torch: every line full 3-D elementwise passes, each product a temporary of its own"""
        cd = cq.data
        Mx = (dy[None, ys, hx:hx + nx + 1] * dz) * u.data[zs, ys, hx:hx + nx + 1]
        Fx = Mx * upwind(Mx, [cd[zs, ys, hx + o:hx + o + nx + 1] for o in range(-3, 3)])
        del Mx
        acc = Fx[:, :, 1:] - Fx[:, :, :-1]
        del Fx
        My = (dx[None, hy:hy + ny + 1, xs] * dz) * v.data[zs, hy:hy + ny + 1, xs]
        Fy = My * upwind(My, [cd[zs, hy + o:hy + o + ny + 1, xs] for o in range(-3, 3)])
        del My
        acc = acc + (Fy[:, 1:, :] - Fy[:, :-1, :])
        del Fy
        Mz = az[None, ys, xs] * w.data[hz:hz + nz + 1, ys, xs]             # faces 1 .. Nz + 1 at index 0 .. Nz
        col = cd[:, ys, xs]
        lv = lambda a, b: col[hz + a - 1:hz + b]                           # levels a .. b (1-based; 0 and Nz + 1 the halo planes)
        C = torch.empty_like(Mz)
        for f in (1, nz + 1):                                              # the walls: the centred mean
            C[f - 1] = 0.5 * (col[hz + f - 2] + col[hz + f - 1])
        for f in (2, nz):                                                  # one face away: the upwind cell
            C[f - 1] = torch.where(Mz[f - 1] >= 0, col[hz + f - 2], col[hz + f - 1])
        for f in (3, nz - 1):                                              # two faces away: R3
            pos = Mz[f - 1] >= 0
            C[f - 1] = face3(torch.where(pos, col[hz + f - 3], col[hz + f]), torch.where(pos, col[hz + f - 2], col[hz + f - 1]),
                             torch.where(pos, col[hz + f - 1], col[hz + f - 2]))
        C[3:nz - 2] = upwind(Mz[3:nz - 2], [lv(4 + o, nz - 2 + o) for o in range(-3, 3)])    # the faces 4 .. Nz - 2: R5
        Fz = Mz * C
        del Mz, C
        acc = acc + (Fz[1:] - Fz[:-1])
        del Fz
        V = az[None, ys, xs] * dz
        out.data[zs, ys, xs] = -(torch.div(one, V) * acc)                 # a division, not a reciprocal approximation

    plan()
    torch.cuda.synchronize()
    if with_torch:
        out_t.data.copy_(G.data)                                   # the halo cells: as the call left them (untouched)
        out_t.data[zs, ys, xs] = 0
        torch_tendency(c, out_t)
        torch.cuda.synchronize()
        res["equals_torch"] = same_bits(torch, G.data, out_t.data)
    fns = {"call_ms": plan, "weno_ms": weno, "copy_ms": lambda: flat[1].copy_(flat[0])}
    if with_torch:
        fns["torch_ms"] = lambda: torch_tendency(c, out_t)
    med, rng = alternating(fns)
    res.update(med)
    res.update(rng)
    res["bytes"] = elems * esz
    res["floor_ms"] = elems * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
    res["call_over_copy_time"] = res["call_ms"] / res["copy_ms"]
    res["call_over_weno_time"] = res["call_ms"] / res["weno_ms"]
    if with_torch:
        res["torch_over_call_time"] = res["torch_ms"] / res["call_ms"]
        res["faster_than_torch_with_disjoint_ranges"] = res["call_ms_range"][1] < res["torch_ms_range"][0]
    if variants:
        # the same call through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        args = plan._call[1]
        plan()
        want = G.data.clone()
        fns, same = {"product": plan}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.WENO_XYZ_SIGNATURES)
            fns[name] = (lambda hd: lambda: _lib.check_weno_xyz(hd.tpg_weno_xyz_tracer_advection_tendency(*args, stream)))(handle)
            G.data.zero_()
            fns[name]()
            same[name] = same_bits(torch, G.data, want)
        med, rng = alternating(fns)
        res["variants_ms"] = med
        res["variants_range_ms"] = rng
        res["variants_same_bits"] = same
        del want
    del plan, weno, u, v, w, c, G, out_t, flat, flush, grid
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_weno_xyz(torch, osg, _lib, dev, variants=(), cases=None, with_torch=True):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        if cases is None or tag in cases:
            out[f"halo{HALO}_{tag}"] = run_case(torch, osg, _lib, dev, SIZE, tdt, variants, with_torch)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call; "
                     "floor = the bytes the call must move (five streams, w one level longer) x sizeof(T) / 8 TB/s; weno = "
                     "tpg_weno_tracer_advection_tendency on the same inputs; copy = dst.copy_(src) on contiguous tensors of half those bytes; torch = "
                     "the rule as torch elementwise passes on slices of the parents; all alternating with the call inside every repetition; "
                     "variants = the call through other builds of the library, alternating; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--weno-xyz-lib"):
        _lib.WENO_XYZ_LIB_PATH = os.path.abspath(arg("--weno-xyz-lib"))
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if arg("--calls-only"):
        tdt = torch.float32 if (cases or ["f64"])[0] == "f32" else torch.float64
        out = run_case(torch, osg, _lib, dev, SIZE, tdt, (), False, calls_only=int(arg("--calls-only")))
    else:
        out = bench_weno_xyz(torch, osg, _lib, dev, variants, cases, "--no-torch" not in sys.argv)
    out["weno_xyz_library"] = os.path.relpath(_lib.WENO_XYZ_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
