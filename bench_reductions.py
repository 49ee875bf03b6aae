"""bench_reductions.py -- the device reductions (tpg_cell_advection_timescale, tpg_field_extrema).

Fields u, v, w, T at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell.  Per case this script times

  * tau_ms   -- tpg_cell_advection_timescale(u, v, w): both launches (the pass and the reduction of the partials) in one stream-event bracket;
  * ext4_ms  -- tpg_field_extrema of (u, v, w, T) in one call: the same bracket;

and, beside each, the three things a reader needs to judge it:

  (a) *_floor_ms        the bytes the pass must read (interior cells x sizeof(T), plus the metric planes for tau) / 8 TB/s;
  (b) *_flat_ms         a flat device read of the same byte count: torch amax of one contiguous tensor of that many bytes;
  (c) *_torch_ms        the torch composition a host of this library would write today, on the same tensors:
                        tau:  (|u| / dx + |v| / dy + |w| / dz).amax() over the interiors, then 1 / it  (each step a full-size temporary);
                        ext:  per field interior.amin(), interior.amax(), interior.abs().amax().

Each figure: median of 10 after 2 dropped, every timed call after a 1 GiB read-only pass (the tensors are 4 - 17 GB: no timed call finds
its input in L2 or the Infinity Cache either way).  The values are compared as well: *_equals_torch says whether the HIP result and the
torch composition agree bit for bit.
Runnable alone:  python bench_reductions.py [--product-lib PATH]   -> one JSON line.
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


def run_case(torch, osg, _lib, dev, size, h, tdt):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v, w, t = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.CenterField(grid)
    for f in (u, v, w, t):
        f.data.uniform_(-1, 1, generator=gen)
    tplan = osg.advection_timescale_plan(u, v, w)
    # (u, v, w, T) in ONE tpg_field_extrema call: w's top level is left to its own group by the package, so the four Nz-level windows
    # of the parents are passed to the C call directly (w: its levels 1..Nz)
    lib = _lib.lib()
    four = [u.data, v.data, w.data, t.data]
    out = torch.empty(12, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.tpg_reduce_workspace_bytes(4, nx, ny, nz)) // 8, dtype=torch.float64, device=dev)
    table = _lib.ptr_table(four)
    stream = _lib.current_stream_ptr(dev)
    ft = _lib.ft_of(tdt)

    def ext4():
        _lib.check(lib.tpg_field_extrema(table, 4, None, None, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, nx, ny, nz, hx, hy, hz, ft, stream))

    inner = lambda f, levels=nz: f.data[hz:hz + levels, hy:hy + ny, hx:hx + nx]
    dx, dy = grid.interior("dx_fc")[None], grid.interior("dy_cf")[None]
    dz = osg.z_face_spacings(grid).to(tdt).to(dev)[:, None, None]

    def tau_torch():
        s = inner(u).abs() / dx + inner(v).abs() / dy + inner(w).abs() / dz
        return 1 / s.amax()

    def ext4_torch():
        return [(x.amin(), x.amax(), x.abs().amax()) for x in (inner(f) for f in (u, v, w, t))]

    cells = nx * ny * nz
    tau_bytes = 3 * cells * esz + 2 * nx * ny * esz
    ext_bytes = 4 * cells * esz
    flat = torch.empty(max(tau_bytes, ext_bytes) // esz, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen)
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def timed(fn):
        res = []
        for _ in range(REPS):
            flush.sum()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1))
        return statistics.median(res[DROP:])

    tplan(); ext4(); torch.cuda.synchronize()                              # warm: code objects, first-call queries
    tau_hip = tplan.result()
    ext_hip = out.tolist()
    tau_ref = float(tau_torch())
    ext_ref = [float(x) for triple in ext4_torch() for x in triple]
    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32",
           "tau_ms": timed(tplan), "tau_bytes": tau_bytes, "tau_floor_ms": tau_bytes / (HBM_PEAK_GBPS * 1e9) * 1e3,
           "tau_flat_ms": timed(lambda: flat[:tau_bytes // esz].amax()), "tau_torch_ms": timed(tau_torch),
           "ext4_ms": timed(ext4), "ext4_bytes": ext_bytes, "ext4_floor_ms": ext_bytes / (HBM_PEAK_GBPS * 1e9) * 1e3,
           "ext4_flat_ms": timed(lambda: flat[:ext_bytes // esz].amax()), "ext4_torch_ms": timed(ext4_torch),
           "tau": tau_hip, "tau_equals_torch": tau_hip == tau_ref, "ext4_equals_torch": ext_hip == ext_ref}
    res["tau_frac_of_hbm_peak"] = res["tau_floor_ms"] / res["tau_ms"]
    res["ext4_frac_of_hbm_peak"] = res["ext4_floor_ms"] / res["ext4_ms"]
    res["tau_over_flat_time"] = res["tau_ms"] / res["tau_flat_ms"]
    res["ext4_over_flat_time"] = res["ext4_ms"] / res["ext4_flat_ms"]
    res["tau_torch_over_hip_time"] = res["tau_torch_ms"] / res["tau_ms"]
    res["ext4_torch_over_hip_time"] = res["ext4_torch_ms"] / res["ext4_ms"]
    del tplan, u, v, w, t, four, flat, flush, grid, dx, dy, dz
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_reductions(torch, osg, _lib, dev):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            out[f"halo{h}_{tag}"] = run_case(torch, osg, _lib, dev, SIZE, h, tdt)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the whole "
                     "C call (the pass and the launch that reduces the partials); floor = algorithmic bytes (interior cells x sizeof(T), "
                     "plus the two metric planes for tau) / 8 TB/s; flat = torch amax of one contiguous tensor of the same bytes; torch = "
                     "the composition a host would write today on the same tensors (tau: abs, /, +, amax, 1 / it; ext4: amin, amax, "
                     "abs().amax() per field)")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    if "--product-lib" in sys.argv:
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--product-lib") + 1])
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_reductions(torch, osg, _lib, dev)
    out["product_library"] = os.path.relpath(_lib.LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
