"""bench_diffusion.py -- the explicit diffusive tendency with its boundary fluxes (tpg_diffusive_tendency).

Fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in every cell, metrics and spacings in [0.5, 2], kappa_z in [0, 2],
a drawn bottom (counts from 0..Nz/2, heights that give them).  Per case this script times, each in a stream-event bracket around the C call:

  * hv_n1, h_n1, v_n1, flux_n1    -- one field, WRITE: both interior groups, each alone, the two flux planes alone;
  * hv_add_n1                     -- ADD: G is read too;
  * hv_field_n1                   -- kappa_z as a FIELD (one more stream);
  * hv_bottom_n1                  -- with the count plane, the bottom height (closed faces) and both flux planes;
  * hv_n2, hv_n4, v_n4            -- n fields in ONE call;  hv_2x1, hv_4x1 -- the same fields in n one-field calls;

and, on the same inputs, in the same process, alternating with them inside every repetition, copy2_ms, copy3_ms: a flat device copy of the
bytes of 2 and 3 streams of the interior (dst.copy_(src) on contiguous tensors, half read, half written): c read and G written; with G
read as well.  No ratio is fixed in advance: the figures are reported as medians with ranges.  Each figure: median of the repetitions kept
after 2 dropped (`*_range`: the least and the greatest of those), every timed entry after a 1 GiB read-only pass.  The order of the entries
ROTATES from one repetition to the next and there are as many kept repetitions as entries.
Runnable alone:  python bench_diffusion.py [--cases halo4_f64,...] [--out PATH]
                 -> one JSON line, also written to PATH (default profiles/diffusion/bench_diffusion.json).
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DROP = 2
SIZE = (NX, NY, NZ)
OUT = os.path.join(ROOT, "profiles", "diffusion", "bench_diffusion.json")
H, V = 1, 2
ADD, WRITE = 0, 1
CONSTANT, FIELD = 0, 2


def run_case(torch, _lib, D, dev, size, h, tdt):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    shape = (nz + 2 * hz, ny + 2 * hy, nx + 2 * hx)
    gen = torch.Generator(device=dev).manual_seed(7)
    rand = lambda s, lo, hi: torch.empty(s, dtype=tdt, device=dev).uniform_(lo, hi, generator=gen)                              # noqa: E731
    fields = [rand(shape, -1, 1) for _ in range(4)]
    G = [rand(shape, -1, 1) for _ in range(4)]
    kfield = rand((nz + 1 + 2 * hz, *shape[1:]), 0, 2)
    planes = {k: rand(shape[1:], 0.5, 2) for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf", "az")}
    top, bottom = [rand(shape[1:], -1, 1) for _ in range(4)], [rand(shape[1:], -1, 1) for _ in range(4)]
    dz_c, dz_f = rand(nz, 0.5, 2), rand(nz + 1, 0.5, 2)
    zc = torch.linspace(-1, 0, 2 * nz + 1, dtype=torch.float64, device=dev)[1::2].to(tdt).contiguous()
    n_cc = torch.randint(0, nz // 2 + 1, shape[1:], dtype=torch.int64, device=dev, generator=gen)
    height = torch.where(n_cc > 0, zc[(n_cc - 1).clamp(min=0)], torch.full_like(zc[n_cc], -2.0)).contiguous()          # zc[n-1] <= h < zc[n]
    counts = n_cc[hy:hy + ny, hx:hx + nx].to(torch.int32).contiguous()
    ft = _lib.ft_of(tdt)
    fn = D.diffusion_lib().tpg_diffusive_tendency
    ptr = lambda t: None if t is None else t.data_ptr()                                                                         # noqa: E731

    def call(which, terms, mode=WRITE, form=CONSTANT, fluxes=False, immersed=False):
        tables = [_lib.ptr_table([fields[q] for q in which]), _lib.ptr_table([G[q] for q in which])]
        flux = [_lib.ptr_table([side[q] for q in which]) if fluxes else None for side in (top, bottom)]
        args = (*tables, len(which), terms, mode, 0.61, ptr(kfield) if form == FIELD else None, 0.37, form, *flux, *(ptr(planes[k]) for k in
                ("dx_fc", "dy_fc", "dx_cf", "dy_cf", "az")), ptr(dz_c), ptr(dz_f), ptr(counts) if immersed else None, 0.0,
                ptr(height) if immersed else None, ptr(zc) if immersed else None, 1, *size, *halo, ft)
        return lambda keep=(tables, flux): D.check_diffusion(fn(*args, _lib.current_stream_ptr(dev)))

    fns = {"hv_n1_ms": call([0], H | V), "h_n1_ms": call([0], H), "v_n1_ms": call([0], V), "flux_n1_ms": call([0], 0, fluxes=True),
           "hv_add_n1_ms": call([0], H | V, ADD), "hv_field_n1_ms": call([0], H | V, form=FIELD),
           "hv_bottom_n1_ms": call([0], H | V, fluxes=True, immersed=True), "v_n4_ms": call([0, 1, 2, 3], V)}
    for n in (2, 4):
        fns[f"hv_n{n}_ms"] = call(list(range(n)), H | V)
        singles = [call([q], H | V) for q in range(n)]
        fns[f"hv_{n}x1_ms"] = lambda singles=singles: [s() for s in singles]
    cells = nx * ny * nz
    for streams in (2, 3):
        half = streams * cells // 2
        pair = (rand(half, -1, 1), torch.empty(half, dtype=tdt, device=dev))
        fns[f"copy{streams}_ms"] = lambda pair=pair: pair[1].copy_(pair[0])
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    fns["hv_bottom_n1_ms"]()
    torch.cuda.synchronize()
    inner = G[0][hz:hz + nz, hy:hy + ny, hx:hx + nx]
    res["finite_share"] = float(torch.isfinite(inner).double().mean())
    res["masked_share"] = float((inner == 0).double().mean())

    def once(f):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    names = list(fns)
    samples = {name: [] for name in names}
    for r in range(len(names) + DROP):                              # after the dropped ones every entry has followed every other entry once
        for name in names[r % len(names):] + names[:r % len(names)]:           # the order rotates: no entry keeps one predecessor
            samples[name].append(once(fns[name]))
    for name, s in samples.items():
        res[name] = statistics.median(s[DROP:])
        res[name + "_range"] = [min(s[DROP:]), max(s[DROP:])]
    res["entries"], res["kept_repetitions"] = len(names), len(names)
    res["bytes_per_stream"] = cells * esz
    res["floor_2_streams_ms"] = 2 * cells * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
    res["hv_n1_over_copy2_time"] = res["hv_n1_ms"] / res["copy2_ms"]
    res["v_n1_over_copy2_time"] = res["v_n1_ms"] / res["copy2_ms"]
    res["hv_add_n1_over_copy3_time"] = res["hv_add_n1_ms"] / res["copy3_ms"]
    for n in (2, 4):
        res[f"hv_n{n}_over_{n}x1_time"] = res[f"hv_n{n}_ms"] / res[f"hv_{n}x1_ms"]
    res["bottom_over_plain_time"] = res["hv_bottom_n1_ms"] / res["hv_n1_ms"]
    del fields, G, kfield, flush
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_diffusion(torch, _lib, D, dev, cases=None):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"halo4_{tag}"
        if cases is None or name in cases:
            out[name] = run_case(torch, _lib, D, dev, SIZE, 4, tdt)
    out["method"] = (f"median of the repetitions kept (as many as entries) after {DROP} dropped, the order of the entries rotating, each entry after a "
                     "1 GiB read-only pass; stream-event bracket around the C call(s); copyN = dst.copy_(src) on contiguous tensors of half the "
                     "bytes of N streams of the interior; floor = 2 streams / 8 TB/s; *_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    from orthogonalsphericalshellgrids.jl_amd import _lib
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None                                        # noqa: E731
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_diffusion(torch, _lib, D, dev, cases)
    out["diffusion_library"] = os.path.relpath(D.DIFFUSION_LIB_PATH, ROOT)
    line = json.dumps(out)
    path = os.path.abspath(arg("--out")) if arg("--out") else OUT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
