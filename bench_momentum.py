"""bench_momentum.py -- the vector-invariant advection tendency of the velocities (tpg_momentum_advection_tendency).

Fields at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell.  Per case this script times, each as the
one launch in a stream-event bracket around the C call,

  * call_ms        -- tpg_momentum_advection_tendency: u, v, w read, Gu, Gv written: 5 3-D streams, w one level longer;

and, beside it, what a reader needs to judge the pass:

  (a) floor_ms     the bytes the call must move x sizeof(T) / 8 TB/s;
  (b) copy_ms      a flat device copy of the same bytes (dst.copy_(src) on contiguous tensors, half the bytes read and half written): THE
                   YARDSTICK of the project's streams, alternating with the call inside every repetition, so that drift of the device lands
                   on both alike;
  (c) torch_ms     what a host has to write without the call: the same rule as torch elementwise passes on slices of the parents (every
                   product, mean, difference and quotient a pass and a temporary of its own), alternating with call_ms;
  equals_torch     whether HIP and (c) agree bit for bit on the whole parents of Gu and Gv (NaNs by NaN-ness), checked before timing;
  variants         with --variants PATH[,PATH...]: the call through each of those builds of the library (the compile-time variants of
                   profiles/momentum/), alternating inside every repetition, with the range of the samples, and whether each leaves the
                   product's bits.

Each figure: median of 10 after 2 dropped (`*_range`: the least and the greatest of the 10), every timed call after a 1 GiB read-only pass
(the tensors are 2 - 4 GB each: no timed call finds its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_momentum.py [--momentum-lib PATH] [--variants PATH,...] [--cases halo4_f64,...] [--no-torch]   -> one JSON line.
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
METRICS = ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff")


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
    Gu, Gv = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v, w):
        f.data.uniform_(-1, 1, generator=gen)
    plan = osg.momentum_advection_plan(u, v, w, Gu, Gv)

    cells = nx * ny * nz
    elems = 4 * cells + nx * ny * (nz + 1)                                  # u, v, Gu, Gv; w one level longer
    half_elems = elems // 2
    flat = [torch.empty(half_elems, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(half_elems, dtype=tdt, device=dev)]
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def copy():
        flat[1].copy_(flat[0])

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
    m = {k: g.arrays[k] for k in METRICS}
    dz = osg.z_all_face_spacings(grid, tdt).to(tdt).to(dev)[:, None, None]
    zs, ys, xs = slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx)
    out_u, out_v = osg.XFaceField(grid), osg.YFaceField(grid)

    def W(p, di=0, dj=0, dk=0, levels=nz):
        """the cells (i + di, j + dj, k + dk) over the interior of a parent (levels: how many) or of a plane"""
        yy, xx = slice(hy + dj, hy + dj + ny), slice(hx + di, hx + di + nx)
        return p[None, yy, xx] if p.dim() == 2 else p[hz + dk:hz + dk + levels, yy, xx]

    def torch_tendency(ou, ov):
        """the rule as a host writes it in torch: every line full 3-D elementwise passes, each operation a temporary of its own"""
        ud, vd, wd = u.data, v.data, w.data
        Z = lambda di, dj: (((W(m["dy_cf"], di, dj) * W(vd, di, dj) - W(m["dy_cf"], di - 1, dj) * W(vd, di - 1, dj))           # noqa: E731
                             - (W(m["dx_fc"], di, dj) * W(ud, di, dj) - W(m["dx_fc"], di, dj - 1) * W(ud, di, dj - 1))) / W(m["az_ff"], di, dj))
        P = lambda di, dj: W(m["dx_cf"], di, dj) * W(vd, di, dj)                                                               # noqa: E731
        Q = lambda di, dj: W(m["dy_fc"], di, dj) * W(ud, di, dj)                                                               # noqa: E731
        A = lambda di, dj: W(m["az_cc"], di, dj) * W(wd, di, dj, 0, nz + 1)                                                    # noqa: E731
        K = lambda di, dj: 0.5 * (0.5 * (W(ud, di, dj) * W(ud, di, dj) + W(ud, di + 1, dj) * W(ud, di + 1, dj))                # noqa: E731
                                  + 0.5 * (W(vd, di, dj) * W(vd, di, dj) + W(vd, di, dj + 1) * W(vd, di, dj + 1)))
        z00, k00, a00 = Z(0, 0), K(0, 0), A(0, 0)
        zb = 0.5 * (z00 + Z(0, 1))
        vh = 0.5 * (0.5 * (P(-1, 0) + P(-1, 1)) + 0.5 * (P(0, 0) + P(0, 1)))
        hu = -((zb * vh) / W(m["dx_fc"]))
        del zb, vh
        bu = (k00 - K(-1, 0)) / W(m["dx_fc"])
        S = (0.5 * (A(-1, 0) + a00)) * ((W(ud, 0, 0, 0, nz + 1) - W(ud, 0, 0, -1, nz + 1)) / dz)
        vu = (0.5 * (S[:-1] + S[1:])) / W(m["az_fc"])
        del S
        ou.data[zs, ys, xs] = -((hu + vu) + bu)
        del hu, vu, bu
        zb = 0.5 * (z00 + Z(1, 0))
        del z00
        uh = 0.5 * (0.5 * (Q(0, -1) + Q(1, -1)) + 0.5 * (Q(0, 0) + Q(1, 0)))
        hv = (zb * uh) / W(m["dy_cf"])
        del zb, uh
        bv = (k00 - K(0, -1)) / W(m["dy_cf"])
        del k00
        R = (0.5 * (A(0, -1) + a00)) * ((W(vd, 0, 0, 0, nz + 1) - W(vd, 0, 0, -1, nz + 1)) / dz)
        del a00
        vv = (0.5 * (R[:-1] + R[1:])) / W(m["az_cf"])
        del R
        ov.data[zs, ys, xs] = -((hv + vv) + bv)

    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    plan()
    torch.cuda.synchronize()
    if with_torch:
        torch_tendency(out_u, out_v)                               # the halo cells of all four: zero, as allocated
        torch.cuda.synchronize()
        res["equals_torch"] = same_bits(torch, Gu.data, out_u.data) and same_bits(torch, Gv.data, out_v.data)
        res["finite_fraction"] = float(torch.isfinite(Gu.data).double().mean())
    fns = {"call_ms": plan, "copy_ms": copy}
    if with_torch:
        fns["torch_ms"] = lambda: torch_tendency(out_u, out_v)
    med, rng = alternating(fns)
    res.update(med)
    res.update(rng)
    res["bytes"] = elems * esz
    res["floor_ms"] = elems * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
    res["call_over_copy_time"] = res["call_ms"] / res["copy_ms"]
    res["call_frac_of_hbm_peak"] = res["floor_ms"] / res["call_ms"]
    if with_torch:
        res["torch_over_call_time"] = res["torch_ms"] / res["call_ms"]
    if variants:
        # the same call through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        args = plan._call[1]
        want = [Gu.data.clone(), Gv.data.clone()]
        fns, same = {"product": plan}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.MOMENTUM_SIGNATURES)
            fns[name] = (lambda hd: lambda: _lib.check_momentum(hd.tpg_momentum_advection_tendency(*args, stream)))(handle)
            Gu.data.zero_()
            Gv.data.zero_()
            fns[name]()
            same[name] = same_bits(torch, Gu.data, want[0]) and same_bits(torch, Gv.data, want[1])
        med, rng = alternating(fns)
        res["variants_ms"] = med
        res["variants_range_ms"] = rng
        res["variants_same_bits"] = same
        del want
    del plan, u, v, w, Gu, Gv, out_u, out_v, flat, flush, grid
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_momentum(torch, osg, _lib, dev, variants=(), cases=None, with_torch=True):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            name = f"halo{h}_{tag}"
            if cases is None or name in cases:
                out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, variants, with_torch)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call; "
                     "floor = the bytes the call must move (5 streams, w one level longer) x sizeof(T) / 8 TB/s; copy = dst.copy_(src) on "
                     "contiguous tensors of half those bytes, alternating with the call inside every repetition; torch = the rule as torch "
                     "elementwise passes on slices of the parents, alternating too; variants = the call through other builds of the library, "
                     "alternating; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None          # noqa: E731
    if arg("--momentum-lib"):
        _lib.MOMENTUM_LIB_PATH = os.path.abspath(arg("--momentum-lib"))
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_momentum(torch, osg, _lib, dev, variants, cases, "--no-torch" not in sys.argv)
    out["momentum_library"] = os.path.relpath(_lib.MOMENTUM_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
