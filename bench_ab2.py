"""bench_ab2.py -- the AB2 step of the velocities with the barotropic forcing, and of the tracers (tpg_ab2_step_velocities, tpg_ab2_step_fields).

Fields at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell; GU, GV on the extended-halo grid of 30
sub-steps (Hy2 = 31).  Per case this script times, each as the one launch in a stream-event bracket around the C call,

  * vel_ms          -- tpg_ab2_step_velocities on (u, v) with the integral into GU, GV and TPG_AB2_STORE_PREVIOUS: 2 x (3 reads + 2 writes) 3-D
                       streams plus the small planes;
  * fields1_ms / fields2_ms -- tpg_ab2_step_fields on one tracer and on two, with TPG_AB2_STORE_PREVIOUS: (3 reads + 2 writes) per tracer;

and, beside them, what a reader needs to judge the passes:

  (a) *_floor_ms    the bytes each call must move x sizeof(T) / 8 TB/s;
  (b) *_copy_ms     a flat device copy of the same bytes (dst.copy_(src) on contiguous tensors, half the bytes read and half written): THE
                    YARDSTICK of the project's in-place streams, alternating with the call inside every repetition, so that drift of the device
                    lands on both alike;
  (c) vel_torch_ms  the parent commit's way of doing the velocity call's work: the rule as torch elementwise passes on the interiors
                    (g = c1 Gn - c2 Gm into a temporary field; u += dt g; Gm = Gn) and tpg_barotropic_mode on the temporaries, alternating with
                    vel_ms; vel_torch_parents_ms: the same passes on the whole contiguous parents (halo cells computed too);
      fields1_torch_ms  the same for one tracer (no integral);
  (d) split_proxy_ms   "segmented step + a separate integral kernel", from below, without building it: vel_noint_ms (the velocity call without
                    GU, GV: the segmented kernel) + tpg_barotropic_mode over (Gu, Gv) and over (Gu_prev, Gv_prev), the four 3-D streams a
                    separate integral kernel has to read again to re-form g (it would also have to run BEFORE the step stores Gm);
  vel_equals_torch / fields_equal_torch   whether HIP and (c) agree bit for bit on every array (NaNs by NaN-ness), checked before timing;
  variants_ms       with --variants PATH[,PATH...]: the calls through each of those builds of the library (the compile-time variants of
                    profiles/ab2/), alternating inside every repetition, and whether each leaves the product's bits.

Each figure: median of 10 after 2 dropped, every timed call after a 1 GiB read-only pass (the tensors are 2 - 4 GB each: no timed call finds
its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_ab2.py [--timestep-lib PATH] [--variants PATH,...] [--cases halo4_f64,...]   -> one JSON line.
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
HY2 = 31
DT, CHI = 600.0, 0.1


def same_bits(torch, x, y):
    ints = torch.int64 if x.dtype == torch.float64 else torch.int32
    return bool(((x.contiguous().view(ints) == y.contiguous().view(ints)) | (x.isnan() & y.isnan())).all())


def run_case(torch, osg, _lib, dev, size, h, tdt, variants):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    ext = osg.with_halo((hx, HY2, hz), grid)
    gen = torch.Generator(device=dev).manual_seed(7)
    new = lambda make: make(grid)
    u, Gu, Gup, Tu = (new(osg.XFaceField) for _ in range(4))       # Tu, Tv: the temporaries of the torch composition
    v, Gv, Gvp, Tv = (new(osg.YFaceField) for _ in range(4))
    c, Gc, Gcp = ([new(osg.CenterField) for _ in range(2)] for _ in range(3))
    GU, GV = osg.Field((osg.Face, osg.Center, None), ext), osg.Field((osg.Center, osg.Face, None), ext)
    TU, TV = osg.Field((osg.Face, osg.Center, None), ext), osg.Field((osg.Center, osg.Face, None), ext)
    for f in (u, Gu, Gup, v, Gv, Gvp, *c, *Gc, *Gcp):
        f.data.uniform_(-1, 1, generator=gen)
    for f in (Gu, Gup, Gv, Gvp, *Gc, *Gcp):
        f.data.mul_(1e-4)                                          # tendencies: repeated steps of 600 s stay finite in Float32
    vel = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gup, Gvp, DT, chi=CHI, GU=GU, GV=GV)
    one = osg.ab2_step_plan(c[:1], Gc[:1], Gcp[:1], DT, chi=CHI)
    two = osg.ab2_step_plan(c, Gc, Gcp, DT, chi=CHI)
    mode = osg.barotropic_mode_plan(Tu, Tv, TU, TV, fill_halos=False)
    noint = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gup, Gvp, DT, chi=CHI)                 # the step without the integral: segments of levels
    mode_n = osg.barotropic_mode_plan(Gu, Gv, TU, TV, fill_halos=False)                     # the reads a separate integral kernel adds
    mode_m = osg.barotropic_mode_plan(Gup, Gvp, TU, TV, fill_halos=False)

    c1 = float((torch.tensor(1.5, dtype=tdt) + torch.tensor(CHI, dtype=tdt)))       # exact values of the type
    c2 = float((torch.tensor(0.5, dtype=tdt) + torch.tensor(CHI, dtype=tdt)))
    dt = float(torch.tensor(DT, dtype=tdt))
    box = (slice(hz, hz + nz), slice(hy, hy + ny), slice(hx, hx + nx))
    whole = (slice(None),) * 3

    def torch_step(x, gn, gm, tmp, where):
        """the rule as a host writes it in torch: every line a full 3-D elementwise pass, each product a temporary of its own"""
        g = tmp.data[where]
        torch.sub(gn.data[where] * c1, gm.data[where] * c2, out=g)
        x.data[where] += g * dt
        gm.data[where].copy_(gn.data[where])

    def torch_velocities(fields, where=box):
        fu, fv, fgup, fgvp = fields
        torch_step(fu, Gu, fgup, Tu, where)
        torch_step(fv, Gv, fgvp, Tv, where)
        mode()

    cells = nx * ny * nz
    flat = [torch.empty(5 * cells, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(5 * cells, dtype=tdt, device=dev)]
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def copy_of(elems):
        return lambda: flat[1][:elems].copy_(flat[0][:elems])

    def once(fn):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def alternating(fns):
        """{name: median}: the calls alternate inside every repetition"""
        samples = {name: [] for name in fns}
        for _ in range(REPS):
            for name, fn in fns.items():
                samples[name].append(once(fn))
        return {name: statistics.median(s[DROP:]) for name, s in samples.items()}

    # bits first: the torch composition on twins of the written arrays against the call, from one start
    twins = [osg.Field(f.loc, grid, data=f.data.clone()) for f in (u, v, Gup, Gvp)]
    torch_velocities(twins)
    vel()
    torch.cuda.synchronize()
    inner2 = lambda f: f.data[0, HY2:HY2 + ny, hx:hx + nx]
    vel_equal = all(same_bits(torch, a.data, b.data) for a, b in zip((u, v, Gup, Gvp), twins)) \
        and same_bits(torch, inner2(GU), inner2(TU)) and same_bits(torch, inner2(GV), inner2(TV))
    ctwin = [osg.Field(f.loc, grid, data=f.data.clone()) for f in (c[0], Gcp[0])]
    torch_step(ctwin[0], Gc[0], ctwin[1], Tu, box)
    one()
    fields_equal = same_bits(torch, c[0].data, ctwin[0].data) and same_bits(torch, Gcp[0].data, ctwin[1].data)
    two(); torch.cuda.synchronize()                                         # warm

    pair_v = alternating({"vel_ms": vel, "vel_copy_ms": copy_of(5 * cells), "vel_torch_ms": lambda: torch_velocities(twins),
                          "vel_noint_ms": noint, "mode_Gn_ms": mode_n, "mode_Gm_ms": mode_m})
    res_p = alternating({"vel_torch_parents_ms": lambda: torch_velocities(twins, whole)})
    pair_1 = alternating({"fields1_ms": one, "fields1_copy_ms": copy_of(5 * cells // 2),
                          "fields1_torch_ms": lambda: torch_step(ctwin[0], Gc[0], ctwin[1], Tu, box)})
    pair_2 = alternating({"fields2_ms": two, "fields2_copy_ms": copy_of(5 * cells)})
    vel_bytes = (10 * nz + 2) * nx * ny * esz
    f1_bytes = 5 * nz * nx * ny * esz
    floor = lambda b: b / (HBM_PEAK_GBPS * 1e9) * 1e3
    res = {"size": list(size), "halo": list(halo), "Hy2": HY2, "eltype": "Float64" if esz == 8 else "Float32", "dt": DT, "chi": CHI,
           "vel_bytes": vel_bytes, "fields1_bytes": f1_bytes, "fields2_bytes": 2 * f1_bytes, **pair_v, **res_p, **pair_1, **pair_2,
           "vel_floor_ms": floor(vel_bytes), "fields1_floor_ms": floor(f1_bytes), "fields2_floor_ms": floor(2 * f1_bytes),
           "vel_equals_torch": vel_equal, "fields_equal_torch": fields_equal}
    res["vel_over_copy_time"] = res["vel_ms"] / res["vel_copy_ms"]
    res["fields1_over_copy_time"] = res["fields1_ms"] / res["fields1_copy_ms"]
    res["fields2_over_copy_time"] = res["fields2_ms"] / res["fields2_copy_ms"]
    res["torch_over_vel_time"] = res["vel_torch_ms"] / res["vel_ms"]
    res["torch_parents_over_vel_time"] = res["vel_torch_parents_ms"] / res["vel_ms"]
    res["torch_over_fields1_time"] = res["fields1_torch_ms"] / res["fields1_ms"]
    res["split_proxy_ms"] = res["vel_noint_ms"] + res["mode_Gn_ms"] + res["mode_Gm_ms"]
    res["split_proxy_over_vel_time"] = res["split_proxy_ms"] / res["vel_ms"]
    res["vel_frac_of_hbm_peak"] = res["vel_floor_ms"] / res["vel_ms"]
    res["fields2_frac_of_hbm_peak"] = res["fields2_floor_ms"] / res["fields2_ms"]
    del twins, ctwin
    if variants:
        # the same calls through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        vargs, fargs = vel._call[1], two._call[1]
        written = (u, v, Gup, Gvp, GU, GV, *c, *Gcp)
        start = [f.data.clone() for f in written]
        vel(); two()
        want = [f.data.clone() for f in written]
        fv, ff, same = {"product": vel}, {"product": two}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.TIMESTEP_SIGNATURES)
            fv[name] = (lambda hd: lambda: _lib.check_timestep(hd.tpg_ab2_step_velocities(*vargs, stream)))(handle)
            ff[name] = (lambda hd: lambda: _lib.check_timestep(hd.tpg_ab2_step_fields(*fargs, stream)))(handle)
            for f, t in zip(written, start):
                f.data.copy_(t)
            fv[name](); ff[name]()
            same[name] = all(same_bits(torch, f.data, t) for f, t in zip(written, want))
        res["variants_vel_ms"] = alternating(fv)
        res["variants_fields2_ms"] = alternating(ff)
        res["variants_same_bits"] = same
        del start, want
    del vel, one, two, mode, noint, mode_n, mode_m, u, v, Gu, Gv, Gup, Gvp, Tu, Tv, c, Gc, Gcp, GU, GV, TU, TV, flat, flush, grid, ext
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_ab2(torch, osg, _lib, dev, variants=(), cases=None):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            name = f"halo{h}_{tag}"
            if cases is None or name in cases:
                out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, variants)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call; "
                     "floors = the bytes each call must move x sizeof(T) / 8 TB/s; copy = dst.copy_(src) on contiguous tensors of half those "
                     "bytes, alternating with the call inside every repetition; torch = the rule as torch elementwise passes on the interiors "
                     "plus tpg_barotropic_mode on the temporaries (the parent commit's way), alternating too; variants = the calls through "
                     "other builds of the library, alternating")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--timestep-lib"):
        _lib.TIMESTEP_LIB_PATH = os.path.abspath(arg("--timestep-lib"))
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_ab2(torch, osg, _lib, dev, variants, cases)
    out["timestep_library"] = os.path.relpath(_lib.TIMESTEP_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
