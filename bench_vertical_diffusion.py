"""bench_vertical_diffusion.py -- the vertically implicit diffusion step (tpg_vertical_implicit_diffusion).

Fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in every cell, spacings in [0.5, 2], kappa in [0, 2].  Per case this
script times, each in a stream-event bracket around the C call(s), the entries `<path>_<what>_ms` with <path> = oc (TPG_VDIFF_ON_CHIP) or st
(TPG_VDIFF_STREAMED):

  * <path>_constant_n1, _profile_n1, _field_n1   -- one field, each kappa form;
  * <path>_constant_n2, _constant_n4             -- n fields in ONE call;  <path>_constant_2x1, _4x1 -- the same fields in n one-field calls;
  * <path>_masked_n1                             -- CONSTANT form with a count plane (counts drawn from 0..Nz/2);

and, on the same inputs, in the same process, alternating with them inside every repetition:

  (1) copy2_ms, copy3_ms, copy4_ms  a flat device copy of the bytes of 2, 3 and 4 streams of the interior (dst.copy_(src) on contiguous
                        tensors, half read, half written): a field read and written; with kappa in FIELD form; with t written and read;
  (2) torch_ms          the rule of include/tripolar_hip_vertical_diffusion.h as per-level torch passes (one field, CONSTANT form, unmasked);
  (3) <variant>_<path>_constant_n1_ms   with --variants: other builds of the library (compile-time variants of profiles/vertical_diffusion/);
  equals_torch          whether HIP and (2) agree bit for bit on the whole parent, checked before timing, for both paths;
  paths_same_bits       whether the two paths left the same bits there;  <variant>_same_bits likewise for a variant.

No ratio is fixed in advance: the figures are reported as medians with ranges.  Each figure: median of the repetitions kept after 2 dropped
(`*_range`: the least and the greatest of those), every timed entry after a 1 GiB read-only pass.  The order of the entries ROTATES from one
repetition to the next and there are as many kept repetitions as entries.  The fields are solved in place from one repetition to the next:
the arithmetic does not depend on the values.
Runnable alone:  python bench_vertical_diffusion.py [--cases halo4_f64,...] [--no-torch] [--variants NAME=PATH,...] [--out PATH]
                 -> one JSON line, also written to PATH (default profiles/vertical_diffusion/bench_vertical_diffusion.json).
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT
from bench_weno import same_bits

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DROP = 2
SIZE = (NX, NY, NZ)
DT = 0.7
KAPPA = 0.37
OUT = os.path.join(ROOT, "profiles", "vertical_diffusion", "bench_vertical_diffusion.json")
CONSTANT, PROFILE, FIELD = 0, 1, 2
PATHS = {"oc": 1, "st": 2}


def torch_rule(torch, x, kappa, dz_c, dz_f, dt, size, halo):
    """the rule for one field, CONSTANT form, unmasked, as torch passes, one level at a time: every torch operation is one IEEE operation of
    the type, in the rule's order; the level-uniform coefficients are 0-d tensors of the type, so nothing is synchronised"""
    (nx, ny, nz), (hx, hy, hz) = size, halo
    T = lambda v: torch.tensor(v, dtype=x.dtype, device=x.device)                                                               # noqa: E731
    dtT, one, kap = T(dt), T(1.0), T(kappa)
    small = T(10.0) * T(torch.finfo(x.dtype).eps)
    L = lambda k: x[hz + k, hy:hy + ny, hx:hx + nx]                                                                             # noqa: E731
    up = [-(dtT * ((kap / dz_c[k]) / dz_f[k + 1])) for k in range(nz - 1)]          # of the face over cell k
    lo = [None] + [-(dtT * ((kap / dz_c[k]) / dz_f[k])) for k in range(1, nz)]       # of the face under cell k
    t = [None] * nz
    beta = one - up[0] if nz > 1 else one
    L(0).copy_(L(0) / beta)
    for k in range(1, nz):
        diag = (one - up[k]) - lo[k] if k + 1 < nz else one - lo[k]
        t[k] = up[k - 1] / beta
        beta = diag - lo[k] * t[k]
        L(k).copy_(torch.where(beta.abs() > small, (L(k) - lo[k] * L(k - 1)) / beta, L(k)))
    for k in range(nz - 2, -1, -1):
        L(k).copy_(L(k) - t[k + 1] * L(k + 1))


def run_case(torch, _lib, dev, size, h, tdt, with_torch, variants):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    shape = (nz + 2 * hz, ny + 2 * hy, nx + 2 * hx)
    gen = torch.Generator(device=dev).manual_seed(7)
    fields = [torch.empty(shape, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen) for _ in range(4)]
    start = fields[0].clone()
    kfield = torch.empty(shape, dtype=tdt, device=dev).uniform_(0, 2, generator=gen)
    kprofile = torch.empty(nz + 1, dtype=tdt, device=dev).uniform_(0, 2, generator=gen)
    dz_c = torch.empty(nz, dtype=tdt, device=dev).uniform_(0.5, 2, generator=gen)
    dz_f = torch.empty(nz + 1, dtype=tdt, device=dev).uniform_(0.5, 2, generator=gen)
    counts = torch.randint(0, nz // 2 + 1, (ny, nx), dtype=torch.int32, device=dev, generator=gen)
    scratch = torch.empty(shape, dtype=tdt, device=dev)
    ft = _lib.ft_of(tdt)
    committed = _lib.vertical_diffusion_lib().tpg_vertical_implicit_diffusion

    def call(fn, which, form, path, masked=False):
        table = _lib.ptr_table([fields[q] for q in which])
        kappa = {CONSTANT: None, PROFILE: kprofile.data_ptr(), FIELD: kfield.data_ptr()}[form]
        args = (table, len(which), kappa, KAPPA if form == CONSTANT else 0.0, form, dz_c.data_ptr(), dz_f.data_ptr(),
                counts.data_ptr() if masked else None, 0.0, DT, scratch.data_ptr() if path == PATHS["st"] else None, path, *size, *halo, ft)
        return lambda: _lib.check_vertical_diffusion(fn(*args, _lib.current_stream_ptr(dev)))

    fns = {}
    for tag, path in PATHS.items():
        for name, form in (("constant", CONSTANT), ("profile", PROFILE), ("field", FIELD)):
            fns[f"{tag}_{name}_n1_ms"] = call(committed, [0], form, path)
        for n in (2, 4):
            fns[f"{tag}_constant_n{n}_ms"] = call(committed, list(range(n)), CONSTANT, path)
            singles = [call(committed, [q], CONSTANT, path) for q in range(n)]
            fns[f"{tag}_constant_{n}x1_ms"] = lambda singles=singles: [s() for s in singles]
        fns[f"{tag}_masked_n1_ms"] = call(committed, [0], CONSTANT, path, masked=True)
    cells = nx * ny * nz
    flat = {}
    for streams in (2, 3, 4):
        half = streams * cells // 2
        flat[streams] = (torch.empty(half, dtype=tdt, device=dev).uniform_(-1, 1, generator=gen), torch.empty(half, dtype=tdt, device=dev))
        fns[f"copy{streams}_ms"] = lambda pair=flat[streams]: pair[1].copy_(pair[0])
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    got = {}
    for tag in PATHS:                                                       # the bits of both paths, and of the torch rule, before timing
        fields[0].copy_(start)
        fns[f"{tag}_constant_n1_ms"]()
        torch.cuda.synchronize()
        got[tag] = fields[0].clone()
    res["paths_same_bits"] = same_bits(torch, got["oc"], got["st"])
    res["finite_share"] = float(torch.isfinite(got["oc"]).double().mean())
    if with_torch:
        fields[0].copy_(start)
        torch_rule(torch, fields[0], KAPPA, dz_c, dz_f, DT, size, halo)
        torch.cuda.synchronize()
        res["equals_torch"] = same_bits(torch, fields[0], got["oc"]) and same_bits(torch, fields[0], got["st"])
        fns["torch_ms"] = lambda: torch_rule(torch, fields[0], KAPPA, dz_c, dz_f, DT, size, halo)
    for name, lib_path in variants.items():
        other = _lib.bind(lib_path, _lib.VERTICAL_DIFFUSION_SIGNATURES).tpg_vertical_implicit_diffusion
        same = True
        for tag, path in PATHS.items():
            run = call(other, [0], CONSTANT, path)
            fields[0].copy_(start)
            run()
            torch.cuda.synchronize()
            same = same and same_bits(torch, fields[0], got[tag])
            fns[f"{name}_{tag}_constant_n1_ms"] = run
        res[name + "_same_bits"] = same
    fields[0].copy_(start)

    def once(fn):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
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
    for tag in PATHS:
        res[f"{tag}_constant_n1_over_copy2_time"] = res[f"{tag}_constant_n1_ms"] / res["copy2_ms"]
        res[f"{tag}_field_n1_over_copy3_time"] = res[f"{tag}_field_n1_ms"] / res["copy3_ms"]
        for n in (2, 4):
            res[f"{tag}_n{n}_over_{n}x1_time"] = res[f"{tag}_constant_n{n}_ms"] / res[f"{tag}_constant_{n}x1_ms"]
        res[f"{tag}_masked_over_unmasked_time"] = res[f"{tag}_masked_n1_ms"] / res[f"{tag}_constant_n1_ms"]
    res["st_constant_n1_over_copy4_time"] = res["st_constant_n1_ms"] / res["copy4_ms"]
    res["oc_over_st_time"] = res["oc_constant_n1_ms"] / res["st_constant_n1_ms"]
    if with_torch:
        res["torch_over_oc_time"] = res["torch_ms"] / res["oc_constant_n1_ms"]
    del fields, kfield, scratch, flat, flush, start, got
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_vertical_diffusion(torch, _lib, dev, cases=None, with_torch=True, variants=None):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"halo4_{tag}"
        if cases is None or name in cases:
            out[name] = run_case(torch, _lib, dev, SIZE, 4, tdt, with_torch, variants or {})
    out["method"] = (f"median of the repetitions kept (as many as entries) after {DROP} dropped, the order of the entries rotating, each entry after a "
                     "1 GiB read-only pass; stream-event bracket around the C call(s); fields solved in place from one repetition to the next; "
                     "copyN = dst.copy_(src) on contiguous tensors of half the bytes of N streams of the interior; torch = the rule as per-level "
                     "torch passes on slices of the parent; variants = other builds of the library; floor = 2 streams / 8 TB/s; "
                     "*_range = the least and the greatest of the kept samples")
    return out


def main():
    import torch
    from orthogonalsphericalshellgrids.jl_amd import _lib
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None                                        # noqa: E731
    cases = arg("--cases").split(",") if arg("--cases") else None
    variants = dict(x.split("=", 1) for x in arg("--variants").split(",")) if arg("--variants") else {}
    variants = {k: os.path.abspath(p) for k, p in variants.items()}
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_vertical_diffusion(torch, _lib, dev, cases, "--no-torch" not in sys.argv, variants)
    out["vertical_diffusion_library"] = os.path.relpath(_lib.VERTICAL_DIFFUSION_LIB_PATH, ROOT)
    out["variants"] = {k: os.path.relpath(p, ROOT) for k, p in variants.items()}
    line = json.dumps(out)
    path = os.path.abspath(arg("--out")) if arg("--out") else OUT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
