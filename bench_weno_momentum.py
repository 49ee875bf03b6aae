"""bench_weno_momentum.py -- the momentum advection tendency with the WENO5-upwinded vorticity term (tpg_weno_momentum_advection_tendency).

Fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in every cell.  Per case this script times, each as the one launch in
a stream-event bracket around the C call,

  * call_ms       -- tpg_weno_momentum_advection_tendency: u, v, w read, Gu, Gv written: 5 3-D streams, w one level longer;

and, beside it, what a reader needs to judge the pass:

  (1) momentum_ms  tpg_momentum_advection_tendency (the enstrophy-conserving, centred vorticity term) on the same inputs;
  (2) copy_ms      a flat device copy of the same bytes (dst.copy_(src) on contiguous tensors, half the bytes read and half written): the
                   yardstick of the project's streams;
  (3) torch_ms     the rule as torch elementwise passes on slices of the parents (Z and K formed once on their extended regions, every
                   product, select and difference a pass and a temporary of its own); THE CONDITION: call_ms is below it with disjoint
                   ranges;
  floor_ms         the bytes the call must move x sizeof(T) / 8 TB/s;
  equals_torch     whether HIP and (3) agree bit for bit on the whole parents of Gu and Gv (NaNs by NaN-ness), checked before timing;
  variants         with --variants PATH[,PATH...]: the call through each of those builds of the library (the compile-time variants of
                   profiles/weno_momentum/), alternating inside every repetition, with the range of the samples, and whether each leaves the
                   product's bits.

All of (1), (2), (3) and the call alternate inside every repetition, so that drift of the device lands on all alike.  Each figure: median of
5 after 2 dropped (`*_range`: the least and the greatest of the 5), every timed call after a 1 GiB read-only pass (the tensors are 2 - 4 GB
each: no timed call finds its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_weno_momentum.py [--weno-momentum-lib PATH] [--variants PATH,...] [--cases halo4_f64,...] [--no-torch]
                 [--calls-only N] [--out PATH]  -> one JSON line, also written to PATH (default profiles/weno_momentum/bench_weno_momentum.json).
`--calls-only N` issues the call N times on the first case and nothing else: the run a counter collection wraps (it writes no file).
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
OUT = os.path.join(ROOT, "profiles", "weno_momentum", "bench_weno_momentum.json")


def torch_rule_tendencies(upwind, ud, vd, wd, m, dzf, size, halo, outu, outv):
    """the rule of include/tripolar_hip_weno_momentum.h as a host writes it in torch, on the parents ud, vd, wd, the metric planes m and
    dzf (Nz + 1, 1, 1), into the interiors of the parents outu, outv: every line full 3-D elementwise passes, each product a temporary of
    its own; Z and K are formed once, on their extended regions"""
    (nx, ny, nz), (hx, hy, hz) = size, halo
    zs, ys, xs = slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx)
    W3 = lambda p, di=0, dj=0: p[zs, hy + dj:hy + dj + ny, hx + di:hx + di + nx]
    W2 = lambda p, di=0, dj=0: p[None, hy + dj:hy + dj + ny, hx + di:hx + di + nx]
    # Z once on the nodes i = -1..Nx+3, j = -1..Ny+3 (1-based), K once on i = 0..Nx, j = 0..Ny
    Sx, Sxm, Sy, Sym = slice(hx - 2, hx + nx + 3), slice(hx - 3, hx + nx + 2), slice(hy - 2, hy + ny + 3), slice(hy - 3, hy + ny + 2)
    Zx = ((m["dy_cf"][None, Sy, Sx] * vd[zs, Sy, Sx] - m["dy_cf"][None, Sy, Sxm] * vd[zs, Sy, Sxm])
          - (m["dx_fc"][None, Sy, Sx] * ud[zs, Sy, Sx] - m["dx_fc"][None, Sym, Sx] * ud[zs, Sym, Sx])) / m["az_ff"][None, Sy, Sx]
    Z = lambda di, dj: Zx[:, 2 + dj:2 + dj + ny, 2 + di:2 + di + nx]
    Kx, Kxp, Ky, Kyp = slice(hx - 1, hx + nx), slice(hx, hx + nx + 1), slice(hy - 1, hy + ny), slice(hy, hy + ny + 1)
    Kk = 0.5 * (0.5 * (ud[zs, Ky, Kx] * ud[zs, Ky, Kx] + ud[zs, Ky, Kxp] * ud[zs, Ky, Kxp])
                + 0.5 * (vd[zs, Ky, Kx] * vd[zs, Ky, Kx] + vd[zs, Kyp, Kx] * vd[zs, Kyp, Kx]))
    K = lambda di, dj: Kk[:, 1 + dj:1 + dj + ny, 1 + di:1 + di + nx]
    P = lambda di, dj: W2(m["dx_cf"], di, dj) * W3(vd, di, dj)
    Q = lambda di, dj: W2(m["dy_fc"], di, dj) * W3(ud, di, dj)
    A = lambda di, dj: W2(m["az_cc"], di, dj) * wd[hz:hz + nz + 1, hy + dj:hy + dj + ny, hx + di:hx + di + nx]
    # u
    vh = 0.5 * (0.5 * (P(-1, 0) + P(-1, 1)) + 0.5 * (P(0, 0) + P(0, 1)))
    vhat = vh / W2(m["dx_fc"])
    del vh
    hu = -(vhat * upwind(vhat, [Z(0, dj) for dj in range(-2, 4)]))
    del vhat
    bu = (K(0, 0) - K(-1, 0)) / W2(m["dx_fc"])
    S = (0.5 * (A(-1, 0) + A(0, 0))) * ((ud[hz:hz + nz + 1, ys, xs] - ud[hz - 1:hz + nz, ys, xs]) / dzf)
    vu = (0.5 * (S[:-1] + S[1:])) / W2(m["az_fc"])
    del S
    outu[zs, ys, xs] = -((hu + vu) + bu)
    del hu, vu, bu
    # v
    uh = 0.5 * (0.5 * (Q(0, -1) + Q(1, -1)) + 0.5 * (Q(0, 0) + Q(1, 0)))
    uhat = uh / W2(m["dy_cf"])
    del uh
    hv = uhat * upwind(uhat, [Z(di, 0) for di in range(-2, 4)])
    del uhat, Zx
    bv = (K(0, 0) - K(0, -1)) / W2(m["dy_cf"])
    R = (0.5 * (A(0, -1) + A(0, 0))) * ((vd[hz:hz + nz + 1, ys, xs] - vd[hz - 1:hz + nz, ys, xs]) / dzf)
    vv = (0.5 * (R[:-1] + R[1:])) / W2(m["az_cf"])
    del R
    outv[zs, ys, xs] = -((hv + vv) + bv)


def run_case(torch, osg, _lib, dev, size, h, tdt, variants, with_torch, calls_only=0):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v, w):
        f.data.uniform_(-1, 1, generator=gen)
    plan = osg.weno_momentum_advection_plan(u, v, w, Gu, Gv)
    if calls_only:
        for _ in range(calls_only):
            plan()
        torch.cuda.synchronize()
        return {"calls": calls_only, "size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    Eu, Ev = osg.XFaceField(grid), osg.YFaceField(grid)
    enstrophy = osg.momentum_advection_plan(u, v, w, Eu, Ev)

    cells = nx * ny * nz
    elems = 4 * cells + nx * ny * (nz + 1)                                  # u, v, Gu, Gv; w one level longer
    half = elems // 2
    flat = [torch.empty(half, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(half, dtype=tdt, device=dev)]
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
    m = {k: g.arrays[k] for k in ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff")}
    dzf = osg.z_all_face_spacings(grid, tdt).to(tdt).to(dev)[:, None, None]
    zs, ys, xs = slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx)
    Tu, Tv = osg.XFaceField(grid), osg.YFaceField(grid)
    upwind = torch_rule(torch, tdt, dev)

    def torch_tendencies(outu, outv):
        torch_rule_tendencies(upwind, u.data, v.data, w.data, m, dzf, size, halo, outu.data, outv.data)

    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    plan()
    torch.cuda.synchronize()
    if with_torch:
        for t, G in ((Tu, Gu), (Tv, Gv)):
            t.data.copy_(G.data)                                    # the halo cells: as the call left them (untouched)
            t.data[zs, ys, xs] = 0
        torch_tendencies(Tu, Tv)
        torch.cuda.synchronize()
        res["equals_torch"] = same_bits(torch, Gu.data, Tu.data) and same_bits(torch, Gv.data, Tv.data)
        res["finite_share"] = float(torch.isfinite(Gu.data[zs, ys, xs]).double().mean())
    fns = {"call_ms": plan, "momentum_ms": enstrophy, "copy_ms": lambda: flat[1].copy_(flat[0])}
    if with_torch:
        fns["torch_ms"] = lambda: torch_tendencies(Tu, Tv)
    med, rng = alternating(fns)
    res.update(med)
    res.update(rng)
    res["bytes"] = elems * esz
    res["floor_ms"] = elems * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
    res["call_over_copy_time"] = res["call_ms"] / res["copy_ms"]
    res["call_over_momentum_time"] = res["call_ms"] / res["momentum_ms"]
    if with_torch:
        res["torch_over_call_time"] = res["torch_ms"] / res["call_ms"]
        res["faster_than_torch_with_disjoint_ranges"] = res["call_ms_range"][1] < res["torch_ms_range"][0]
    if variants:
        # the same call through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        args = plan._call[1]
        plan()
        want = [Gu.data.clone(), Gv.data.clone()]
        fns, same = {"product": plan}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.WENO_MOMENTUM_SIGNATURES)
            fns[name] = (lambda hd: lambda: _lib.check_weno_momentum(hd.tpg_weno_momentum_advection_tendency(*args, stream)))(handle)
            Gu.data.zero_()
            Gv.data.zero_()
            fns[name]()
            same[name] = same_bits(torch, Gu.data, want[0]) and same_bits(torch, Gv.data, want[1])
        med, rng = alternating(fns)
        res["variants_ms"] = med
        res["variants_range_ms"] = rng
        res["variants_same_bits"] = same
        del want
    del plan, enstrophy, u, v, w, Gu, Gv, Eu, Ev, Tu, Tv, flat, flush, grid
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_weno_momentum(torch, osg, _lib, dev, variants=(), cases=None, with_torch=True):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"halo4_{tag}"
        if cases is None or name in cases:
            out[name] = run_case(torch, osg, _lib, dev, SIZE, 4, tdt, variants, with_torch)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call; "
                     "floor = the bytes the call must move (5 streams, w one level longer) x sizeof(T) / 8 TB/s; momentum = "
                     "tpg_momentum_advection_tendency on the same inputs; copy = dst.copy_(src) on contiguous tensors of half those bytes; torch = "
                     "the rule as torch elementwise passes on slices of the parents; all alternating with the call inside every repetition; "
                     "variants = the call through other builds of the library, alternating; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--weno-momentum-lib"):
        _lib.WENO_MOMENTUM_LIB_PATH = os.path.abspath(arg("--weno-momentum-lib"))
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
        out = bench_weno_momentum(torch, osg, _lib, dev, variants, cases, "--no-torch" not in sys.argv)
    out["weno_momentum_library"] = os.path.relpath(_lib.WENO_MOMENTUM_LIB_PATH, ROOT)
    line = json.dumps(out)
    if not arg("--calls-only"):
        path = os.path.abspath(arg("--out")) if arg("--out") else OUT
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
