"""bench_barotropic.py -- the barotropic mode and the split-explicit velocity correction (tpg_barotropic_mode, tpg_barotropic_correction).

Fields u, v at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell; the 2-D fields on the extended-halo
grid of 30 sub-steps (Hy2 = 31).  Per case this script times

  * mode_ms        -- tpg_barotropic_mode on (u, v): the one launch in a stream-event bracket;
  * mode_fill_ms   -- the plan a host runs per step: the launch and the halo fill of (Ubar, Vbar);
  * corr_ms        -- tpg_barotropic_correction on (u, v) with Ubar, Vbar given: the one launch;
  * corr_fill_ms   -- the launch and the halo fill of (u, v);

and, beside them, what a reader needs to judge the passes:

  (a) mode_floor_ms / corr_floor_ms   the bytes each pass must move (the mode: 2 Nz interior planes read, 2 written; the correction: 2 Nz read
                    and written, 4 planes read) x sizeof(T) / 8 TB/s;
  (b) extrema_ms    tpg_field_extrema over the same (u, v), an existing pass that reads exactly the same interior once: THE YARDSTICK of the
                    mode, alternating with mode_ms inside every repetition, so that drift of the device lands on both alike;
  (c) copy_ms       a flat device copy of the correction's bytes (dst.copy_(src) on contiguous tensors of 2 Nz interior planes): THE
                    YARDSTICK of the correction, alternating with corr_ms;
  (d) mode_torch_ms / corr_torch_ms   the rules as a host of this library writes them without the calls: the per-level loops of torch passes;
  mode_equals_torch / corr_equals_torch   whether HIP and (d) agree bit for bit on the whole interior (NaNs by NaN-ness), checked before timing;
  variants_ms       with --variants PATH[,PATH...]: both calls through each of those builds of the library (the compile-time variants of
                    profiles/barotropic/), alternating inside every repetition, and whether each leaves the product's bits.

Each figure: median of 10 after 2 dropped, every timed call after a 1 GiB read-only pass (the tensors are 2 - 4 GB each: no timed call finds
its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_barotropic.py [--barotropic-lib PATH] [--variants PATH,...] [--cases halo4_f64,...]   -> one JSON line.
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
HY2 = 31


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
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    plane = lambda x: osg.Field((osg.Face, osg.Center, None) if x else (osg.Center, osg.Face, None), ext)
    U, V, Ub, Vb = plane(1), plane(0), plane(1), plane(0)
    for f in (u, v, U, V):
        f.data.uniform_(-1, 1, generator=gen)
    mode = osg.barotropic_mode_plan(u, v, Ub, Vb, fill_halos=False)
    mode_fill = osg.barotropic_mode_plan(u, v, Ub, Vb)
    corr = osg.barotropic_correction_plan(u, v, U, V, Ub, Vb, fill_halos=False)
    corr_fill = osg.barotropic_correction_plan(u, v, U, V, Ub, Vb)
    extrema = osg.extrema_plan([u, v])

    dz = [float(d) for d in osg.z_center_spacings(grid, tdt)]     # exact values of the type
    depth = osg.column_depth_table(grid, tdt)[0].to(tdt).to(dev)          # a 0-dim tensor: torch divides by it (a Python float it would multiply by 1 / H)
    rows, cols, rows2 = slice(hy, hy + ny), slice(hx, hx + nx), slice(HY2, HY2 + ny)
    inner2 = lambda f: f.data[0, rows2, cols]

    def torch_mode():
        """the rule, level by level: a product and an add per level and field, each a full-plane torch pass with a temporary"""
        out = []
        for f in (u, v):
            acc = dz[0] * f.data[hz, rows, cols]
            for k in range(1, nz):
                acc = acc + dz[k] * f.data[hz + k, rows, cols]
            out.append(acc)
        return out

    def torch_corr(fu, fv):
        for f, t, tb in ((fu, U, Ub), (fv, V, Vb)):
            c = (inner2(t) - inner2(tb)) / depth
            for k in range(nz):
                f[hz + k, rows, cols] += c
        return fu, fv

    cells = nx * ny * nz
    flat = [torch.empty(2 * cells, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(2 * cells, dtype=tdt, device=dev)]
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

    mode_fill(); extrema(); mode(); torch.cuda.synchronize()               # warm: code objects, first-call queries; the bare mode last
    want = torch_mode()
    mode_equal = same_bits(torch, inner2(Ub), want[0]) and same_bits(torch, inner2(Vb), want[1])
    del want
    twin = torch_corr(u.data.clone(), v.data.clone())
    corr()
    corr_equal = same_bits(torch, u.data, twin[0]) and same_bits(torch, v.data, twin[1])
    corr_fill(); mode(); torch.cuda.synchronize()                          # Ubar, Vbar as the rule leaves them again
    pair_m = alternating({"mode_ms": mode, "extrema_ms": extrema})
    pair_c = alternating({"corr_ms": corr, "copy_ms": lambda: flat[1].copy_(flat[0])})
    mode_bytes, corr_bytes = (2 * nz + 2) * nx * ny * esz, (4 * nz + 4) * nx * ny * esz
    res = {"size": list(size), "halo": list(halo), "Hy2": HY2, "eltype": "Float64" if esz == 8 else "Float32",
           "mode_bytes": mode_bytes, "corr_bytes": corr_bytes, **pair_m, **pair_c,
           "mode_fill_ms": timed(mode_fill), "corr_fill_ms": timed(corr_fill),
           "mode_floor_ms": mode_bytes / (HBM_PEAK_GBPS * 1e9) * 1e3, "corr_floor_ms": corr_bytes / (HBM_PEAK_GBPS * 1e9) * 1e3,
           "mode_torch_ms": timed(torch_mode), "corr_torch_ms": timed(lambda: torch_corr(*twin)),
           "mode_equals_torch": mode_equal, "corr_equals_torch": corr_equal}
    del twin
    res["mode_over_extrema_time"] = res["mode_ms"] / res["extrema_ms"]
    res["corr_over_copy_time"] = res["corr_ms"] / res["copy_ms"]
    res["mode_frac_of_hbm_peak"] = res["mode_floor_ms"] / res["mode_ms"]
    res["corr_frac_of_hbm_peak"] = res["corr_floor_ms"] / res["corr_ms"]
    res["torch_over_mode_time"] = res["mode_torch_ms"] / res["mode_ms"]
    res["torch_over_corr_time"] = res["corr_torch_ms"] / res["corr_ms"]
    if variants:
        # the same calls through other builds of the library: compile-time variants, alternating inside every repetition
        stream = _lib.current_stream_ptr(dev)
        margs, cargs = mode._call[1], corr._call[1]
        mode()
        want_bar = (inner2(Ub).clone(), inner2(Vb).clone())
        start = (u.data.clone(), v.data.clone())
        corr()
        want = (u.data.clone(), v.data.clone())
        fm, fc, same = {}, {}, {}
        for path in variants:
            name = os.path.basename(path)
            handle = _lib.bind(path, _lib.BAROTROPIC_SIGNATURES)
            fm[name] = (lambda hd: lambda: _lib.check_barotropic(hd.tpg_barotropic_mode(*margs, stream)))(handle)
            fc[name] = (lambda hd: lambda: _lib.check_barotropic(hd.tpg_barotropic_correction(*cargs, stream)))(handle)
            u.data.copy_(start[0])
            v.data.copy_(start[1])
            Ub.data.zero_()
            Vb.data.zero_()
            fm[name]()
            ok = same_bits(torch, inner2(Ub), want_bar[0]) and same_bits(torch, inner2(Vb), want_bar[1])
            fc[name]()
            same[name] = ok and same_bits(torch, u.data, want[0]) and same_bits(torch, v.data, want[1])
        res["variants_mode_ms"] = alternating(fm)
        res["variants_corr_ms"] = alternating(fc)
        res["variants_same_bits"] = same
        del want_bar, start, want
    del mode, mode_fill, corr, corr_fill, extrema, u, v, U, V, Ub, Vb, flat, flush, grid, ext
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_barotropic(torch, osg, _lib, dev, variants=(), cases=None):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            name = f"halo{h}_{tag}"
            if cases is None or name in cases:
                out[name] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, variants)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call "
                     "(mode_ms, corr_ms) or the plan with the outputs' halo fill (mode_fill_ms, corr_fill_ms); floors = the bytes each pass must "
                     "move x sizeof(T) / 8 TB/s; extrema = tpg_field_extrema over the same (u, v), alternating with mode_ms inside every "
                     "repetition; copy = dst.copy_(src) on contiguous tensors of 2 Nz interior planes, alternating with corr_ms; torch = the "
                     "rules as per-level loops of torch passes; variants = both calls through other builds of the library, alternating")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None
    if arg("--barotropic-lib"):
        _lib.BAROTROPIC_LIB_PATH = os.path.abspath(arg("--barotropic-lib"))
    variants = [os.path.abspath(p) for p in arg("--variants").split(",")] if arg("--variants") else []
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_barotropic(torch, osg, _lib, dev, variants, cases)
    out["barotropic_library"] = os.path.relpath(_lib.BAROTROPIC_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
