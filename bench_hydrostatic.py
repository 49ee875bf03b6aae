"""bench_hydrostatic.py -- the Coriolis and hydrostatic pressure-gradient tendencies accumulated into Gu, Gv (tpg_hydrostatic_tendencies).

Fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in every cell; ADD mode, both terms, the enstrophy-conserving scheme,
no p_out: seven 3-D streams (u, v, b, Gu and Gv read, Gu and Gv written).  Per case this script times, each in a stream-event bracket
around the C call,

  * call_ms            -- tpg_hydrostatic_tendencies;

and, on the same inputs, in the same process, alternating with it inside every repetition:

  (1) copy_ms           a flat device copy of the same bytes (dst.copy_(src) on contiguous tensors, half read, half written);
  (2) torch_ms          the rule of include/tripolar_hip_hydrostatic.h as per-level torch passes on slices of the parents;
  (3) momentum_ms       tpg_momentum_advection_tendency, the call whose output this one continues;
  (4) <variant>_ms      with --variants: other builds of libtripolar_hip_hydrostatic.so (compile-time variants of profiles/hydrostatic/);
  floor_ms              the bytes / 8 TB/s;
  equals_torch          whether HIP and (2) agree bit for bit on the whole parents of Gu and Gv (NaNs by NaN-ness), checked before timing;
  <variant>_same_bits   whether a variant leaves the bits of the committed build in Gu and Gv.

No ratio is fixed in advance: the figures are reported as medians with ranges.  Each figure: median of the repetitions kept after 2 dropped
(`*_range`: the least and the greatest of those), every timed call after a 1 GiB read-only pass.  The order of the entries ROTATES from
one repetition to the next and there are at least as many kept repetitions as entries (5 at the least): the time of a call depends on
what ran before it (two runs with a fixed order ranked the same two builds oppositely, profiles/hydrostatic/README.md).
Runnable alone:  python bench_hydrostatic.py [--cases halo4_f64,...] [--no-torch] [--variants NAME=PATH,...] [--out PATH]
                 -> one JSON line, also written to PATH (default profiles/hydrostatic/bench_hydrostatic.json).
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
OUT = os.path.join(ROOT, "profiles", "hydrostatic", "bench_hydrostatic.json")


def torch_rule_add(torch, u, v, b, Gu, Gv, f, m, dz, size, halo):
    """Gu = (Gu + cu) - px, Gv = (Gv - cv) - py of the enstrophy-conserving scheme as torch passes, one level at a time, top-down; every
    torch operation is one IEEE operation of the type, in the rule's order"""
    (nx, ny, nz), (hx, hy, hz) = size, halo
    W = lambda p, di=0, dj=0: p[hy + dj:hy + dj + ny, hx + di:hx + di + nx]                                                    # noqa: E731
    fu, fv = 0.5 * (W(f) + W(f, 0, 1)), 0.5 * (W(f) + W(f, 1, 0))
    PH = None
    for k in range(nz - 1, -1, -1):
        x = (0.5 * (b[hz + k] + b[hz + k + 1])) * dz[k + 1]
        PH = -x if PH is None else PH - x
        px = (W(PH) - W(PH, -1, 0)) / W(m["dx_fc"])
        py = (W(PH) - W(PH, 0, -1)) / W(m["dy_cf"])
        P, Q = m["dx_cf"] * v[hz + k], m["dy_fc"] * u[hz + k]
        vh = 0.5 * (0.5 * (W(P, -1, 0) + W(P, -1, 1)) + 0.5 * (W(P) + W(P, 0, 1)))
        uh = 0.5 * (0.5 * (W(Q, 0, -1) + W(Q, 1, -1)) + 0.5 * (W(Q) + W(Q, 1, 0)))
        cu, cv = (fu * vh) / W(m["dx_fc"]), (fv * uh) / W(m["dy_cf"])
        gu, gv = W(Gu[hz + k]), W(Gv[hz + k])
        gu.copy_((gu + cu) - px)
        gv.copy_((gv - cv) - py)


def run_case(torch, osg, _lib, dev, size, h, tdt, with_torch, variants):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w, b = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.CenterField(grid)
    Gu, Gv = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v, w, b, Gu, Gv):
        f.data.uniform_(-1, 1, generator=gen)
    start = [Gu.data.clone(), Gv.data.clone()]
    coriolis = osg.HydrostaticSphericalCoriolis()
    plan = osg.hydrostatic_tendencies_plan(u, v, Gu, Gv, coriolis=coriolis, b=b)
    Eu, Ev = osg.XFaceField(grid), osg.YFaceField(grid)
    momentum = osg.momentum_advection_plan(u, v, w, Eu, Ev)

    cells = nx * ny * nz
    moved = 7 * cells                                                       # u, v, b, Gu, Gv read; Gu, Gv written
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
        names = list(fns)
        reps = max(REPS, len(names) + DROP)                         # after the dropped ones every entry has followed every other entry once
        for r in range(reps):
            for name in names[r % len(names):] + names[:r % len(names)]:       # the order rotates: no entry keeps one predecessor
                samples[name].append(once(fns[name]))
        return ({name: statistics.median(s[DROP:]) for name, s in samples.items()},
                {name + "_range": [min(s[DROP:]), max(s[DROP:])] for name, s in samples.items()})

    def reset():
        for f, t in zip((Gu, Gv), start):
            f.data.copy_(t)

    g = getattr(grid, "underlying_grid", grid)
    m = {k: g.arrays[k] for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf")}
    f_ff = osg.coriolis_parameter(grid, coriolis, tdt)
    dz = osg.z_all_face_spacings(grid, tdt).to(tdt).to(dev)
    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    plan()
    torch.cuda.synchronize()
    got = [Gu.data.clone(), Gv.data.clone()]
    zs, ys, xs = slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx)
    res["finite_share"] = float(torch.isfinite(got[0][zs, ys, xs]).double().mean())
    fns = {"call_ms": plan, "copy_ms": lambda: flat[1].copy_(flat[0]), "momentum_ms": momentum}
    if with_torch:
        reset()
        torch_rule_add(torch, u.data, v.data, b.data, Gu.data, Gv.data, f_ff, m, dz, size, halo)
        torch.cuda.synchronize()
        res["equals_torch"] = same_bits(torch, Gu.data, got[0]) and same_bits(torch, Gv.data, got[1])
        fns["torch_ms"] = lambda: torch_rule_add(torch, u.data, v.data, b.data, Gu.data, Gv.data, f_ff, m, dz, size, halo)
    fn0, args = plan._call
    for name, path in variants.items():
        other = _lib.bind(path, _lib.HYDROSTATIC_SIGNATURES).tpg_hydrostatic_tendencies
        run = lambda other=other: _lib.check_hydrostatic(other(*args, _lib.current_stream_ptr(dev)))                           # noqa: E731
        reset()
        run()
        torch.cuda.synchronize()
        res[name + "_same_bits"] = same_bits(torch, Gu.data, got[0]) and same_bits(torch, Gv.data, got[1])
        fns[name + "_ms"] = run
    reset()
    med, rng = alternating(fns)
    res.update(med)
    res.update(rng)
    res["bytes"] = moved * esz
    res["floor_ms"] = moved * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
    res["call_over_copy_time"] = res["call_ms"] / res["copy_ms"]
    res["call_over_momentum_time"] = res["call_ms"] / res["momentum_ms"]
    if with_torch:
        res["torch_over_call_time"] = res["torch_ms"] / res["call_ms"]
    del plan, momentum, u, v, w, b, Gu, Gv, Eu, Ev, flat, flush, grid, start, got
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_hydrostatic(torch, osg, _lib, dev, cases=None, with_torch=True, variants=None):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"halo4_{tag}"
        if cases is None or name in cases:
            out[name] = run_case(torch, osg, _lib, dev, SIZE, 4, tdt, with_torch, variants or {})
    out["method"] = (f"median of the repetitions kept (at least {REPS - DROP}, as many as entries) after {DROP} dropped, the order of the entries rotating, each call after a 1 GiB read-only pass; stream-event bracket around the C call; "
                     "ADD mode, both terms, enstrophy-conserving, no p_out, no mask; bytes = 7 streams of the interior, floor = bytes / 8 TB/s; "
                     "copy = dst.copy_(src) on contiguous tensors of half those bytes; torch = the rule as per-level torch passes on slices of "
                     "the parents; momentum = tpg_momentum_advection_tendency on the same u, v; variants = other builds of the library; all "
                     "alternating with the call inside every repetition; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None                                        # noqa: E731
    cases = arg("--cases").split(",") if arg("--cases") else None
    variants = dict(x.split("=", 1) for x in arg("--variants").split(",")) if arg("--variants") else {}
    variants = {k: os.path.abspath(p) for k, p in variants.items()}
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_hydrostatic(torch, osg, _lib, dev, cases, "--no-torch" not in sys.argv, variants)
    out["hydrostatic_library"] = os.path.relpath(_lib.HYDROSTATIC_LIB_PATH, ROOT)
    out["variants"] = {k: os.path.relpath(p, ROOT) for k, p in variants.items()}
    line = json.dumps(out)
    path = os.path.abspath(arg("--out")) if arg("--out") else OUT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
