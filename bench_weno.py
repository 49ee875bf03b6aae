"""bench_weno.py -- the WENO5 flux-form advection tendency of the tracers (tpg_weno_tracer_advection_tendency).

Fields at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell, with n = 1, 2 and 4 tracers in a call.
Per case and n this script times, each as the one launch in a stream-event bracket around the C call,

  * call{n}_ms      -- tpg_weno_tracer_advection_tendency on n tracers: u, v, w and n tracers read, n tendencies written: (3 + 2n) 3-D
                       streams, w one level longer;

and, beside them, what a reader needs to judge the pass:

  (1) centered{n}_ms  tpg_tracer_advection_tendency (`centered2`) on the same fields: the second-order scheme's kernel, stream-bound;
  (2) copy{n}_ms      a flat device copy of the same bytes (dst.copy_(src) on contiguous tensors, half the bytes read and half written): the
                      yardstick of the project's streams;
  (3) torch1_ms       the rule for one tracer as torch elementwise passes on slices of the parents (every product, select and difference a
                      pass and a temporary of its own); THE CONDITION: call1_ms is below it with disjoint ranges;
      momentum_ms     tpg_momentum_advection_tendency on the same grid (the other VALU-bound tendency), for the "under 2x" statement of
                      DESIGN.md 6;
  floor{n}_ms         the bytes the call must move x sizeof(T) / 8 TB/s;
  equals_torch        whether HIP and (3) agree bit for bit on the whole parent of G (NaNs by NaN-ness), checked before timing;
  variants            with --variants PATH[,PATH...]: the 1-, 2- and 4-tracer calls through each of those builds of the library (the
                      compile-time variants of profiles/weno/), alternating inside every repetition, with the range of the samples, and
                      whether each leaves the product's bits.

All of (1), (2), (3) and the call alternate inside every repetition, so that drift of the device lands on all alike.  Each figure: median of
5 after 2 dropped (`*_range`: the least and the greatest of the 5), every timed call after a 1 GiB read-only pass (the tensors are 2 - 4 GB
each: no timed call finds its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_weno.py [--weno-lib PATH] [--variants PATH,...] [--cases halo4_f64,...] [--no-torch] [--calls-only N]  -> one JSON line.
`--calls-only N` issues the one-tracer call N times on the first case and nothing else: the run a counter collection wraps.
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPS, DROP = 7, 2
SIZE = (NX, NY, NZ)
TRACERS = (1, 2, 4)


def same_bits(torch, x, y):
    ints = torch.int64 if x.dtype == torch.float64 else torch.int32
    return bool(((x.contiguous().view(ints) == y.contiguous().view(ints)) | (x.isnan() & y.isnan())).all())


def torch_rule(torch, tdt, dev):
    """the rule of include/tripolar_hip_weno.h as torch passes: (face_value, upwind) on tensors, the constants computed in the type"""
    t = lambda x: torch.tensor(x, dtype=tdt, device=dev)
    K = lambda n, d: t(n) / t(d)
    k13, k76, k116, k56, k16, k1312, k310, k35, k110 = K(1, 3), K(7, 6), K(11, 6), K(5, 6), K(1, 6), K(13, 12), K(3, 10), K(3, 5), K(1, 10)
    eps, quarter = t(1e-8), t(0.25)

    def face_value(q0, q1, q2, q3, q4):
        p2 = (k13 * q0 - k76 * q1) + k116 * q2
        p1 = (k56 * q2 - k16 * q1) + k13 * q3
        p0 = (k13 * q2 + k56 * q3) - k16 * q4
        s2, d2 = (q0 - 2 * q1) + q2, (q0 - 4 * q1) + 3 * q2
        s1, d1 = (q1 - 2 * q2) + q3, q1 - q3
        s0, d0 = (q2 - 2 * q3) + q4, (3 * q2 - 4 * q3) + q4
        b2 = k1312 * (s2 * s2) + quarter * (d2 * d2)
        b1 = k1312 * (s1 * s1) + quarter * (d1 * d1)
        b0 = k1312 * (s0 * s0) + quarter * (d0 * d0)
        del s2, d2, s1, d1, s0, d0
        tau = (b0 - b2).abs()
        r0, r1, r2 = tau / (b0 + eps), tau / (b1 + eps), tau / (b2 + eps)
        del b0, b1, b2, tau
        a0, a1, a2 = k310 * (1 + r0 * r0), k35 * (1 + r1 * r1), k110 * (1 + r2 * r2)
        del r0, r1, r2
        return ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2)

    def upwind(M, x):
        pos = M >= 0
        return face_value(*(torch.where(pos, x[n], x[5 - n]) for n in range(5)))

    return upwind


def run_case(torch, osg, _lib, dev, size, h, tdt, variants, with_torch, calls_only=0):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, G = ([osg.CenterField(grid) for _ in range(max(TRACERS))] for _ in range(2))
    for f in (u, v, w, *c):
        f.data.uniform_(-1, 1, generator=gen)
    plans = {n: osg.weno_tracer_advection_plan(c[:n], u, v, w, G[:n]) for n in TRACERS}
    if calls_only:
        for _ in range(calls_only):
            plans[1]()
        torch.cuda.synchronize()
        return {"calls": calls_only, "size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    centered = {n: osg.tracer_advection_plan(c[:n], u, v, w, G[:n]) for n in TRACERS}
    Gu, Gv = osg.XFaceField(grid), osg.YFaceField(grid)
    momentum = osg.momentum_advection_plan(u, v, w, Gu, Gv)

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
    upwind = torch_rule(torch, tdt, dev)

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
        fns = {f"call{n}_ms": plans[n], f"centered{n}_ms": centered[n], f"copy{n}_ms": copy_of(n)}
        if n == 1:
            fns["momentum_ms"] = momentum
            if with_torch:
                fns["torch1_ms"] = lambda: torch_tendency(c[0], out_t)
        med, rng = alternating(fns)
        res.update(med)
        res.update(rng)
        res[f"bytes{n}"] = elems[n] * esz
        res[f"floor{n}_ms"] = floor(elems[n] * esz)
        res[f"call{n}_over_copy_time"] = res[f"call{n}_ms"] / res[f"copy{n}_ms"]
        res[f"call{n}_over_centered_time"] = res[f"call{n}_ms"] / res[f"centered{n}_ms"]
    res["call1_over_momentum_time"] = res["call1_ms"] / res["momentum_ms"]
    if with_torch:
        res["torch_over_call1_time"] = res["torch1_ms"] / res["call1_ms"]
        res["faster_than_torch_with_disjoint_ranges"] = res["call1_ms_range"][1] < res["torch1_ms_range"][0]
    res["call2_over_twice_call1"] = res["call2_ms"] / (2 * res["call1_ms"])
    res["call4_over_four_call1"] = res["call4_ms"] / (4 * res["call1_ms"])
    if variants:
        # the same calls through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        args = {n: plans[n]._call[1] for n in TRACERS}
        for n in TRACERS:
            plans[n]()
        want = [f.data.clone() for f in G]
        fns, same = {f"product_{n}": plans[n] for n in TRACERS}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.WENO_SIGNATURES)
            for n in TRACERS:
                fns[f"{name}_{n}"] = (lambda hd, a: lambda: _lib.check_weno(hd.tpg_weno_tracer_advection_tendency(*a, stream)))(handle, args[n])
            for f in G:
                f.data.zero_()
            fns[f"{name}_{max(TRACERS)}"]()
            same[name] = all(same_bits(torch, f.data, t) for f, t in zip(G, want))
        med, rng = alternating(fns)
        res["variants_ms"] = med
        res["variants_range_ms"] = rng
        res["variants_same_bits"] = same
        del want
    del plans, centered, momentum, u, v, w, c, G, Gu, Gv, out_t, flat, flush, grid
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_weno(torch, osg, _lib, dev, variants=(), cases=None, with_torch=True):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            name = f"halo{h}_{tag}"
            if cases is None or name in cases:
                out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, variants, with_torch)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call; "
                     "floors = the bytes each call must move ((3 + 2n) streams, w one level longer) x sizeof(T) / 8 TB/s; centered = "
                     "tpg_tracer_advection_tendency on the same fields; copy = dst.copy_(src) on contiguous tensors of half those bytes; torch = "
                     "the rule as torch elementwise passes on slices of the parents; momentum = tpg_momentum_advection_tendency on the same grid; "
                     "all alternating with the call inside every repetition; variants = the 1-, 2- and 4-tracer calls through other builds of "
                     "the library, alternating; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--weno-lib"):
        _lib.WENO_LIB_PATH = os.path.abspath(arg("--weno-lib"))
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if arg("--calls-only"):
        tag = (cases or ["halo4_f64"])[0]
        tdt = torch.float64 if tag.endswith("f64") else torch.float32
        out = run_case(torch, osg, _lib, dev, SIZE, int(tag[4]), tdt, (), False, calls_only=int(arg("--calls-only")))
    else:
        out = bench_weno(torch, osg, _lib, dev, variants, cases, "--no-torch" not in sys.argv)
    out["weno_library"] = os.path.relpath(_lib.WENO_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
