"""bench_weno_vs.py -- the momentum advection tendency of the drivers' WENOVectorInvariant(vorticity_order = 5)
(tpg_weno_vs_momentum_advection_tendency): what VelocityStencil smoothness of the vorticity reconstruction costs.

The protocol of bench_weno_vi.py: fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in every cell.  Per case this
script times, each in a stream-event bracket around the C call (two launches on one stream),

  * call_ms            -- tpg_weno_vs_momentum_advection_tendency;

and, on the same inputs, in the same process, alternating with it inside every repetition:

  (1) weno_vi_ms        tpg_weno_vi_momentum_advection_tendency (DefaultStencil smoothness): existing code, the yardstick.  The two calls
                        differ in their first launch only;
  (2) torch_ms          the rule as torch elementwise passes on slices of the parents (bench_weno_vi.torch_rule_tendencies with w5v);
  (3) copy_ms           a flat device copy of the bytes the call must move (dst.copy_(src) on contiguous tensors, half read, half written);
  floor_ms              those bytes x sizeof(T) / 8 TB/s;
  equals_torch          whether HIP and (2) agree bit for bit on the whole parents of Gu and Gv (NaNs by NaN-ness), checked before timing;
  differs_from_weno_vi  whether the call's Gu differs from weno_vi's anywhere (it must: the stencil shows in the bits).

No ratio is fixed in advance: the figures are reported as medians with ranges.  Each figure: median of 5 after 2 dropped (`*_range`: the
least and the greatest of the 5), every timed call after a 1 GiB read-only pass.
Runnable alone:  python bench_weno_vs.py [--cases halo4_f64,...] [--no-torch] [--library PATH] [--out PATH]
                 -> one JSON line, also written to PATH (default profiles/weno_vs/bench_weno_vs.json).
`--library PATH` binds another build of libtripolar_hip_weno_vs.so (a compile-time variant of profiles/weno_vs/).
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT
from bench_weno import same_bits
from bench_weno_vi import torch_rule, torch_rule_tendencies

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPS, DROP = 7, 2
SIZE = (NX, NY, NZ)
OUT = os.path.join(ROOT, "profiles", "weno_vs", "bench_weno_vs.json")


def torch_w5v(torch, tdt, dev):
    """W5V of include/tripolar_hip_weno_vs.h as torch passes, the constants computed in the type"""
    t = lambda x: torch.tensor(x, dtype=tdt, device=dev)
    K = lambda n, d: t(n) / t(d)
    k13, k76, k116, k56, k16, k1312, k310, k35, k110 = K(1, 3), K(7, 6), K(11, 6), K(5, 6), K(1, 6), K(13, 12), K(3, 10), K(3, 5), K(1, 10)
    eps, quarter = t(1e-8), t(0.25)

    def indicators(t0, t1, t2, t3, t4):
        s2, d2 = (t0 - 2 * t1) + t2, (t0 - 4 * t1) + 3 * t2
        s1, d1 = (t1 - 2 * t2) + t3, t1 - t3
        s0, d0 = (t2 - 2 * t3) + t4, (3 * t2 - 4 * t3) + t4
        return (k1312 * (s2 * s2) + quarter * (d2 * d2), k1312 * (s1 * s1) + quarter * (d1 * d1), k1312 * (s0 * s0) + quarter * (d0 * d0))

    def w5v(q, a, b):
        q0, q1, q2, q3, q4 = q
        p2 = (k13 * q0 - k76 * q1) + k116 * q2
        p1 = (k56 * q2 - k16 * q1) + k13 * q3
        p0 = (k13 * q2 + k56 * q3) - k16 * q4
        (a2, a1, a0), (c2, c1, c0) = indicators(*a), indicators(*b)
        b2, b1, b0 = 0.5 * (a2 + c2), 0.5 * (a1 + c1), 0.5 * (a0 + c0)
        del a2, a1, a0, c2, c1, c0
        tau = (b0 - b2).abs()
        r0, r1, r2 = tau / (b0 + eps), tau / (b1 + eps), tau / (b2 + eps)
        del b0, b1, b2, tau
        w0, w1, w2 = k310 * (1 + r0 * r0), k35 * (1 + r1 * r1), k110 * (1 + r2 * r2)
        del r0, r1, r2
        return ((w0 * p0 + w1 * p1) + w2 * p2) / ((w0 + w1) + w2)

    return w5v


def run_case(torch, osg, _lib, dev, size, h, tdt, with_torch):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v, w):
        f.data.uniform_(-1, 1, generator=gen)
    plan = osg.weno_vs_momentum_advection_plan(u, v, w, Gu, Gv)
    Eu, Ev = osg.XFaceField(grid), osg.YFaceField(grid)
    older = osg.weno_vi_momentum_advection_plan(u, v, w, Eu, Ev)

    cells = nx * ny * nz
    elems = 4 * cells + nx * ny * (nz + 1)                                  # u, v, Gu, Gv; w one level longer
    moved = elems + 4 * cells                                               # hu, hv written by the first launch and read back by the second
    half = moved // 2
    flat = [torch.empty(half, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(half, dtype=tdt, device=dev)]
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def once(fn):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def alternating(fns):
        samples = {name: [] for name in fns}
        for _ in range(REPS):
            for name, fn in fns.items():
                samples[name].append(once(fn))
        return ({name: statistics.median(s[DROP:]) for name, s in samples.items()},
                {name + "_range": [min(s[DROP:]), max(s[DROP:])] for name, s in samples.items()})

    g = getattr(grid, "underlying_grid", grid)
    m = {k: g.arrays[k] for k in ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff")}
    dzc = osg.z_center_spacings(grid, tdt).to(tdt).to(dev)[:, None, None]
    zs, ys, xs = slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx)
    Tu, Tv = osg.XFaceField(grid), osg.YFaceField(grid)
    rule, w5v = torch_rule(torch, tdt, dev), torch_w5v(torch, tdt, dev)

    def torch_tendencies(outu, outv):
        torch_rule_tendencies(torch, rule, u.data, v.data, w.data, m, dzc, size, halo, outu.data, outv.data, w5v=w5v)

    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    plan()
    older()
    torch.cuda.synchronize()
    res["differs_from_weno_vi"] = not same_bits(torch, Gu.data, Eu.data)
    if with_torch:
        for t, G in ((Tu, Gu), (Tv, Gv)):
            t.data.copy_(G.data)                                    # the halo cells: as the call left them (untouched)
            t.data[zs, ys, xs] = 0
        torch_tendencies(Tu, Tv)
        torch.cuda.synchronize()
        res["equals_torch"] = same_bits(torch, Gu.data, Tu.data) and same_bits(torch, Gv.data, Tv.data)
        res["finite_share"] = float(torch.isfinite(Gu.data[zs, ys, xs]).double().mean())
    fns = {"call_ms": plan, "weno_vi_ms": older, "copy_ms": lambda: flat[1].copy_(flat[0])}
    if with_torch:
        fns["torch_ms"] = lambda: torch_tendencies(Tu, Tv)
    med, rng = alternating(fns)
    res.update(med)
    res.update(rng)
    res["bytes"] = moved * esz
    res["floor_ms"] = moved * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
    res["call_over_copy_time"] = res["call_ms"] / res["copy_ms"]
    res["call_over_weno_vi_time"] = res["call_ms"] / res["weno_vi_ms"]
    if with_torch:
        res["torch_over_call_time"] = res["torch_ms"] / res["call_ms"]
    del plan, older, u, v, w, Gu, Gv, Eu, Ev, Tu, Tv, flat, flush, grid
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_weno_vs(torch, osg, _lib, dev, cases=None, with_torch=True):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"halo4_{tag}"
        if cases is None or name in cases:
            out[name] = run_case(torch, osg, _lib, dev, SIZE, 4, tdt, with_torch)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call "
                     "(two launches); bytes = 5 streams (w one level longer) plus hu, hv written and read back once, floor = bytes / 8 TB/s; "
                     "weno_vi = tpg_weno_vi_momentum_advection_tendency on the same inputs; copy = dst.copy_(src) on contiguous tensors of half "
                     "those bytes; torch = the rule as torch elementwise passes on slices of the parents; all alternating with the call inside "
                     "every repetition; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    cases = arg("--cases").split(",") if arg("--cases") else None
    if arg("--library"):                                           # a compile-time variant of profiles/weno_vs/ (make WENO_VS_TAG=...)
        _lib.WENO_VS_LIB_PATH = os.path.abspath(arg("--library"))
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_weno_vs(torch, osg, _lib, dev, cases, "--no-torch" not in sys.argv)
    out["weno_vs_library"] = os.path.relpath(_lib.WENO_VS_LIB_PATH, ROOT)
    line = json.dumps(out)
    path = os.path.abspath(arg("--out")) if arg("--out") else OUT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
