"""bench_vorticity.py -- the vertical vorticity pass (tpg_vertical_vorticity).

Fields u, v, zeta at 3600 x 1800 x 75, halo 4 and (5, 5, 5), Float64 and Float32, random values in every cell, on the grid's own metric arrays.
Per case this script times

  * hip_ms        -- tpg_vertical_vorticity alone: the one launch in a stream-event bracket;
  * hip_fill_ms   -- the plan a host runs per output: that launch and zeta's own halo fill;

and, beside them, what a reader needs to judge the pass:

  (a) floor_ms    the bytes the pass must move (2 streams read, 1 written: 3 x interior cells x sizeof(T), plus the three metric planes) / 8 TB/s;
  (b) flat_ms     a flat device pass of the same stream shape: torch.add(a, b, out=c) on contiguous tensors of the interior's size;
  (c) torch_ms    the torch composition of the rule on the same tensors, as a host of this library writes it without the call: four products,
                  three differences and a quotient over the interior views, each a full-size pass with a temporary;
  equals_torch    whether the HIP result and (c) agree bit for bit on the whole interior (NaNs by NaN-ness);
  levels_ms       the kernel with a work item walking 1 (= the level-outer order), 8, 16, 25 and all 75 levels, through the test library's
                  TPG_VORTICITY_LEVELS (tools/libtripolar_hip_operators_test.so), the settings alternating inside every repetition (--no-levels leaves this out).

Each figure: median of 10 after 2 dropped, every timed call after a 1 GiB read-only pass (the tensors are 2 - 4 GB each: no timed call finds
its input in L2 or the Infinity Cache either way).
Runnable alone:  python bench_vorticity.py [--operators-lib PATH] [--no-levels]   -> one JSON line.
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
LEVELS = (1, 8, 16, 25, 75)


def same_bits(torch, x, y):
    ints = torch.int64 if x.dtype == torch.float64 else torch.int32
    return bool(((x.contiguous().view(ints) == y.contiguous().view(ints)) | (x.isnan() & y.isnan())).all())


def run_case(torch, osg, _lib, dev, size, h, tdt, levels):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    grid = osg.TripolarGrid(osg.GPU(dev.index), tdt, size=size, halo=halo, z=(-4000, 0))
    gen = torch.Generator(device=dev).manual_seed(7)
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v])
    zeta = osg.Field((osg.Face, osg.Face, osg.Center), grid)
    plan = osg.vorticity_plan(u, v, zeta)
    bare = osg.vorticity_plan(u, v, zeta, fill_halos=False)

    win = lambda t, di=0, dj=0: t[..., hy + dj:hy + dj + ny, hx + di:hx + di + nx]
    inner = lambda f, di=0, dj=0: win(f.data[hz:hz + nz], di, dj)
    dx, dy, az = grid.arrays["dx_fc"], grid.arrays["dy_cf"], grid.arrays["az_ff"]

    def composition():
        a = win(dy) * inner(v)
        b = win(dy, -1, 0) * inner(v, -1, 0)
        c = win(dx) * inner(u)
        d = win(dx, 0, -1) * inner(u, 0, -1)
        return ((a - b) - (c - d)) / win(az)

    cells = nx * ny * nz
    nbytes = 3 * cells * esz + 3 * nx * ny * esz
    flat = [torch.empty(cells, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen) for _ in range(2)] + [torch.empty(cells, dtype=tdt, device=dev)]
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def once(fn):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn):
        return statistics.median([once(fn) for _ in range(REPS)][DROP:])

    plan(); bare(); torch.cuda.synchronize()                               # warm: code objects, first-call queries
    ref = composition()
    equal = same_bits(torch, inner(zeta), ref)
    del ref
    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32", "bytes": nbytes,
           "hip_ms": timed(bare), "hip_fill_ms": timed(plan), "floor_ms": nbytes / (HBM_PEAK_GBPS * 1e9) * 1e3,
           "flat_ms": timed(lambda: torch.add(flat[0], flat[1], out=flat[2])), "torch_ms": timed(composition), "equals_torch": equal}
    res["frac_of_hbm_peak"] = res["floor_ms"] / res["hip_ms"]
    res["over_flat_time"] = res["hip_ms"] / res["flat_ms"]
    res["torch_over_hip_time"] = res["torch_ms"] / res["hip_ms"]
    if levels:
        # the same call through the test library, whose TPG_VORTICITY_LEVELS sets the levels a work item walks; the settings alternate
        # inside every repetition, so that drift of the device lands on all of them alike
        from tools import testlib
        tl = testlib.operators_lib()
        _, args = bare._call
        stream = _lib.current_stream_ptr(dev)

        def setting(n):
            os.environ["TPG_VORTICITY_LEVELS"] = str(n)
            assert tl.tpg_reload_config() == 0

        want = inner(zeta).clone()
        samples = {n: [] for n in levels}
        same = {}
        for rep in range(REPS):
            for n in levels:
                setting(n)
                if rep == 0:
                    zeta.data.zero_()
                    _lib.check_operators(tl.tpg_vertical_vorticity(*args, stream))
                    same[n] = same_bits(torch, inner(zeta), want)
                samples[n].append(once(lambda: _lib.check_operators(tl.tpg_vertical_vorticity(*args, stream))))
        os.environ.pop("TPG_VORTICITY_LEVELS", None)
        assert tl.tpg_reload_config() == 0
        res["levels_ms"] = {str(n): statistics.median(samples[n][DROP:]) for n in levels}
        res["levels_same_bits"] = all(same.values())
        del want
    del plan, bare, u, v, zeta, flat, flush, grid, dx, dy, az
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_vorticity(torch, osg, _lib, dev, levels=LEVELS):
    out = {}
    for h in (4, 5):
        for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            out[f"halo{h}_{tag}"] = run_case(torch, osg, _lib, dev, SIZE, h, tdt, levels)
    out["method"] = (f"median of {REPS - DROP} after {DROP} dropped, each call after a 1 GiB read-only pass; stream-event bracket around the C call "
                     "(hip_ms) or the plan with zeta's halo fill (hip_fill_ms); floor = (3 x interior cells + 3 metric planes) x sizeof(T) / "
                     "8 TB/s; flat = torch.add(a, b, out=c) on contiguous tensors of the interior's size; torch = the composition of the rule "
                     "on the same tensors (4 products, 3 differences, 1 quotient, each a full-size pass with a temporary); levels_ms = the "
                     "kernel with a work item walking that many levels (1 = level-outer order), settings alternating inside every repetition")
    return out


def main():
    import torch
    import orthogonalsphericalshellgrids.jl_amd as osg
    from orthogonalsphericalshellgrids.jl_amd import _lib
    if "--operators-lib" in sys.argv:
        _lib.OPERATORS_LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--operators-lib") + 1])
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_vorticity(torch, osg, _lib, dev, () if "--no-levels" in sys.argv else LEVELS)
    out["operators_library"] = os.path.relpath(_lib.OPERATORS_LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
