"""bench_weno_vi.py -- the momentum advection tendency with upwinding in every term (tpg_weno_vi_momentum_advection_tendency).

Fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in every cell.  Per case this script times, each in a stream-event
bracket around the C call (two launches on one stream),

  * call_ms            -- tpg_weno_vi_momentum_advection_tendency: u, v, w read, Gu, Gv written, and Gu, Gv read back once by the second
                          launch: 5 3-D streams, w one level longer, plus one more pass over Gu and Gv in each direction;

and, on the same inputs, alternating with it inside every repetition:

  (1) weno_momentum_ms  tpg_weno_momentum_advection_tendency (the WENO vorticity flux with the centred vertical term and kinetic-energy
                        gradient): what the new terms cost beside the built ones;
  (2) torch_ms          the rule as torch elementwise passes on slices of the parents (every product, select and difference a pass and a
                        temporary of its own; the z-faces plane by plane);
  (3) copy_ms           a flat device copy of the bytes the call must move (dst.copy_(src) on contiguous tensors, half read, half written);
  floor_ms              those bytes x sizeof(T) / 8 TB/s;
  equals_torch          whether HIP and (2) agree bit for bit on the whole parents of Gu and Gv (NaNs by NaN-ness), checked before timing.

No ratio is fixed in advance: the figures are reported as medians with ranges.  Each figure: median of 5 after 2 dropped (`*_range`: the
least and the greatest of the 5), every timed call after a 1 GiB read-only pass.
Runnable alone:  python bench_weno_vi.py [--cases halo4_f64,...] [--no-torch] [--calls-only N] [--out PATH]
                 -> one JSON line, also written to PATH (default profiles/weno_vi/bench_weno_vi.json).
`--calls-only N` issues the call N times on the first case and nothing else: the run a counter collection wraps (it writes no file).
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT
from bench_weno import same_bits

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPS, DROP = 7, 2
SIZE = (NX, NY, NZ)
OUT = os.path.join(ROOT, "profiles", "weno_vi", "bench_weno_vi.json")


def torch_rule(torch, tdt, dev):
    """(c4, w5f, r3) of include/tripolar_hip_weno_vi.h as torch passes, the constants computed in the type"""
    t = lambda x: torch.tensor(x, dtype=tdt, device=dev)
    K = lambda n, d: t(n) / t(d)
    k13, k76, k116, k56, k16, k1312, k310, k35, k110 = K(1, 3), K(7, 6), K(11, 6), K(5, 6), K(1, 6), K(13, 12), K(3, 10), K(3, 5), K(1, 10)
    k712, k112, k23 = K(7, 12), K(1, 12), K(2, 3)
    eps, quarter = t(1e-8), t(0.25)

    def c4(a, b, c, d):
        return k712 * (b + c) - k112 * (a + d)

    def w5f(q, s):
        q0, q1, q2, q3, q4 = q
        t0, t1, t2, t3, t4 = s
        p2 = (k13 * q0 - k76 * q1) + k116 * q2
        p1 = (k56 * q2 - k16 * q1) + k13 * q3
        p0 = (k13 * q2 + k56 * q3) - k16 * q4
        s2, d2 = (t0 - 2 * t1) + t2, (t0 - 4 * t1) + 3 * t2
        s1, d1 = (t1 - 2 * t2) + t3, t1 - t3
        s0, d0 = (t2 - 2 * t3) + t4, (3 * t2 - 4 * t3) + t4
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

    def r3(q0, q1, q2):
        p1 = 1.5 * q1 - 0.5 * q0
        p0 = 0.5 * (q1 + q2)
        e1, e0 = q1 - q0, q2 - q1
        b1, b0 = e1 * e1, e0 * e0
        tau = (b0 - b1).abs()
        r0, r1 = tau / (b0 + eps), tau / (b1 + eps)
        a0, a1 = k23 * (1 + r0 * r0), k13 * (1 + r1 * r1)
        return (a0 * p0 + a1 * p1) / (a0 + a1)

    return c4, w5f, r3


def torch_rule_tendencies(torch, rule, ud, vd, wd, m, dzc, size, halo, outu, outv, w5v=None):
    """the rule of include/tripolar_hip_weno_vi.h as a host writes it in torch, on the parents ud, vd, wd, the metric planes m and dzc
    (Nz, 1, 1), into the interiors of the parents outu, outv: every line full 3-D elementwise passes, each product a temporary of its own;
    the shared quantities are formed once, on whole planes.  With `w5v` (bench_weno_vs.py): the rule of include/tripolar_hip_weno_vs.h, zr
    is w5v(Z window, UB window, VB window)"""
    c4, w5f, r3 = rule
    (nx, ny, nz), (hx, hy, hz) = size, halo
    zs, ys, xs = slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx)
    W = lambda p, di=0, dj=0: p[..., hy + dj:hy + dj + ny, hx + di:hx + di + nx]                 # the cells (i + di, j + dj) of whole planes
    M = lambda name, di=0, dj=0: W(m[name], di, dj)[None]
    ul, vl = ud[zs], vd[zs]

    def upwind(vel, q, s):
        pos = vel >= 0
        return w5f([torch.where(pos, q[n], q[5 - n]) for n in range(5)], [torch.where(pos, s[n], s[5 - n]) for n in range(5)])

    def zface(x, Mz):
        """C at the nz + 1 faces of the interior columns of the parent x, plane by plane"""
        col = x[:, ys, xs]
        level = lambda n: col[hz + n - 1]
        out = torch.empty_like(Mz)
        for f in range(1, nz + 2):
            dist, pos = min(f - 1, nz + 1 - f), Mz[f - 1] >= 0
            if dist == 0:
                out[f - 1] = 0.5 * (level(f - 1) + level(f))
            elif dist == 1:
                out[f - 1] = torch.where(pos, level(f - 1), level(f))
            elif dist == 2:
                out[f - 1] = r3(torch.where(pos, level(f - 2), level(f + 1)), torch.where(pos, level(f - 1), level(f)),
                                torch.where(pos, level(f), level(f - 1)))
            else:
                c = [level(f + o) for o in range(-3, 3)]
                q = [torch.where(pos, c[n], c[5 - n]) for n in range(5)]
                out[f - 1] = w5f(q, q)
        return out

    # the built vorticity term: Z once on the nodes i = -1..Nx+3, j = -1..Ny+3
    Sx, Sxm, Sy, Sym = slice(hx - 2, hx + nx + 3), slice(hx - 3, hx + nx + 2), slice(hy - 2, hy + ny + 3), slice(hy - 3, hy + ny + 2)
    Zx = ((m["dy_cf"][None, Sy, Sx] * vd[zs, Sy, Sx] - m["dy_cf"][None, Sy, Sxm] * vd[zs, Sy, Sxm])
          - (m["dx_fc"][None, Sy, Sx] * ud[zs, Sy, Sx] - m["dx_fc"][None, Sym, Sx] * ud[zs, Sym, Sx])) / m["az_ff"][None, Sy, Sx]
    Z = lambda di, dj: Zx[:, 2 + dj:2 + dj + ny, 2 + di:2 + di + nx]
    P = lambda di, dj: M("dx_cf", di, dj) * W(vl, di, dj)
    Q = lambda di, dj: M("dy_fc", di, dj) * W(ul, di, dj)
    vh = 0.5 * (0.5 * (P(-1, 0) + P(-1, 1)) + 0.5 * (P(0, 0) + P(0, 1)))
    vhat = vh / M("dx_fc")
    UB = lambda di, dj: 0.5 * (W(ul, di, dj - 1) + W(ul, di, dj))
    VB = lambda di, dj: 0.5 * (W(vl, di - 1, dj) + W(vl, di, dj))

    def zr(pos, zw, nodes):
        pick = lambda x: [torch.where(pos, x[n], x[5 - n]) for n in range(5)]
        q = pick(zw)
        return w5f(q, q) if w5v is None else w5v(q, pick([UB(di, dj) for di, dj in nodes]), pick([VB(di, dj) for di, dj in nodes]))

    zw = [Z(0, dj) for dj in range(-2, 4)]
    hu = -(vhat * zr(vhat >= 0, zw, [(0, dj) for dj in range(-2, 4)]))
    uh = 0.5 * (0.5 * (Q(0, -1) + Q(1, -1)) + 0.5 * (Q(0, 0) + Q(1, 0)))
    uhat = uh / M("dy_cf")
    zw = [Z(di, 0) for di in range(-2, 4)]
    hv = uhat * zr(uhat >= 0, zw, [(di, 0) for di in range(-2, 4)])
    del Zx, zw, vh, uh, vhat, uhat
    # the shared quantities of the new terms, on whole planes less one column and one row
    FX = (m["dy_fc"][None] * ul) * dzc
    FY = (m["dx_cf"][None] * vl) * dzc
    DU = (FX[:, :, 1:] - FX[:, :, :-1])[:, :-1, :]
    DV = (FY[:, 1:, :] - FY[:, :-1, :])[:, :, :-1]
    DS = DU + DV
    del FX, FY
    HU, HV = 0.5 * (ul * ul), 0.5 * (vl * vl)
    DKU = HU[:, :, 1:] - HU[:, :, :-1]
    DKV = HV[:, 1:, :] - HV[:, :-1, :]
    XKV = HV[:, :, 1:] - HV[:, :, :-1]                              # at column index c: XKV[c + 1]
    XKU = HU[:, 1:, :] - HU[:, :-1, :]                              # at row index r: XKU[r + 1]
    SU = 0.5 * (ul[:, :, :-1] + ul[:, :, 1:])
    SV = 0.5 * (vl[:, :-1, :] + vl[:, 1:, :])
    A = m["az_cc"][None] * wd[hz:hz + nz + 1]
    uu, vv = W(ul), W(vl)
    # u
    dvs = c4(*(W(DV, di, 0) for di in range(-2, 2)))
    dur = upwind(uu, [W(DU, di, 0) for di in range(-3, 3)], [W(DS, di, 0) for di in range(-3, 3)])
    Wu = c4(*(W(A, di, 0) for di in range(-2, 2)))
    FZ = Wu * zface(ud, Wu)
    vu = (uu * (dvs + dur) + (FZ[1:] - FZ[:-1])) / (M("az_fc") * dzc)
    del dvs, dur, Wu, FZ
    kus = c4(*(W(XKV, -1, dj) for dj in range(-1, 3)))
    kur = upwind(uu, [W(DKU, di, 0) for di in range(-3, 3)], [W(SU, di, 0) for di in range(-3, 3)])
    bu = (kur + kus) / M("dx_fc")
    outu[zs, ys, xs] = -((hu + vu) + bu)
    del hu, vu, bu, kus, kur
    # v
    dus = c4(*(W(DU, 0, dj) for dj in range(-2, 2)))
    dvr = upwind(vv, [W(DV, 0, dj) for dj in range(-3, 3)], [W(DS, 0, dj) for dj in range(-3, 3)])
    Wv = c4(*(W(A, 0, dj) for dj in range(-2, 2)))
    FZ = Wv * zface(vd, Wv)
    vvert = (vv * (dus + dvr) + (FZ[1:] - FZ[:-1])) / (M("az_cf") * dzc)
    del dus, dvr, Wv, FZ
    kvs = c4(*(W(XKU, di, -1) for di in range(-1, 3)))
    kvr = upwind(vv, [W(DKV, 0, dj) for dj in range(-3, 3)], [W(SV, 0, dj) for dj in range(-3, 3)])
    bv = (kvr + kvs) / M("dy_cf")
    outv[zs, ys, xs] = -((hv + vvert) + bv)


def run_case(torch, osg, _lib, dev, size, h, tdt, with_torch, calls_only=0):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v, w):
        f.data.uniform_(-1, 1, generator=gen)
    plan = osg.weno_vi_momentum_advection_plan(u, v, w, Gu, Gv)
    if calls_only:
        for _ in range(calls_only):
            plan()
        torch.cuda.synchronize()
        return {"calls": calls_only, "size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    Eu, Ev = osg.XFaceField(grid), osg.YFaceField(grid)
    older = osg.weno_momentum_advection_plan(u, v, w, Eu, Ev)

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
    rule = torch_rule(torch, tdt, dev)

    def torch_tendencies(outu, outv):
        torch_rule_tendencies(torch, rule, u.data, v.data, w.data, m, dzc, size, halo, outu.data, outv.data)

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
    fns = {"call_ms": plan, "weno_momentum_ms": older, "copy_ms": lambda: flat[1].copy_(flat[0])}
    if with_torch:
        fns["torch_ms"] = lambda: torch_tendencies(Tu, Tv)
    med, rng = alternating(fns)
    res.update(med)
    res.update(rng)
    res["bytes"] = moved * esz
    res["floor_ms"] = moved * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
    res["call_over_copy_time"] = res["call_ms"] / res["copy_ms"]
    res["call_over_weno_momentum_time"] = res["call_ms"] / res["weno_momentum_ms"]
    if with_torch:
        res["torch_over_call_time"] = res["torch_ms"] / res["call_ms"]
    del plan, older, u, v, w, Gu, Gv, Eu, Ev, Tu, Tv, flat, flush, grid
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_weno_vi(torch, osg, _lib, dev, cases=None, with_torch=True):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"halo4_{tag}"
        if cases is None or name in cases:
            out[name] = run_case(torch, osg, _lib, dev, SIZE, 4, tdt, with_torch)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call "
                     "(two launches); bytes = 5 streams (w one level longer) plus hu, hv written and read back once, floor = bytes / 8 TB/s; "
                     "weno_momentum = tpg_weno_momentum_advection_tendency on the same inputs; copy = dst.copy_(src) on contiguous tensors of half "
                     "those bytes; torch = the rule as torch elementwise passes on slices of the parents; all alternating with the call inside "
                     "every repetition; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if arg("--calls-only"):
        tag = (cases or ["halo4_f64"])[0]
        tdt = torch.float64 if tag.endswith("f64") else torch.float32
        out = run_case(torch, osg, _lib, dev, SIZE, int(tag[4]), tdt, False, calls_only=int(arg("--calls-only")))
    else:
        out = bench_weno_vi(torch, osg, _lib, dev, cases, "--no-torch" not in sys.argv)
    out["weno_vi_library"] = os.path.relpath(_lib.WENO_VI_LIB_PATH, ROOT)
    line = json.dumps(out)
    if not arg("--calls-only"):
        path = os.path.abspath(arg("--out")) if arg("--out") else OUT
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
