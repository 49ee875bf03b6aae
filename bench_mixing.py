"""bench_mixing.py -- the vertical mixing diffusivities (tpg_convective_adjustment_diffusivities, tpg_ri_based_diffusivities).

Fields at 3600 x 1800 x 75, halo 4, Float64 and Float32, random values in [-1, 1] in every cell, dz_f in [0.5, 2], the previous
diffusivities in [0, 2].  Per case this script times, each in a stream-event bracket around the call:

  * ca_ms                 -- convective adjustment, all four outputs: b read, four parents written (5 streams);
  * ri_ms, ri_prev_ms     -- the Ri rule, all four outputs, without and with the time average: 7 and 9 streams;
  * torch_ca_ms, torch_ri_ms, torch_ri_prev_ms -- the same rule written as shifted-slice torch passes on the same inputs (what a host had
                             to write before): its outputs are asserted to equal the call's BIT FOR BIT on the evaluated faces before
                             anything is timed;
  * copy5_ms, copy7_ms, copy9_ms -- a flat device copy of the bytes of as many streams of the interior (dst.copy_(src) on contiguous
                             tensors, half read, half written).

No ratio is fixed in advance: the figures are reported as medians with ranges.  FIVE alternating runs are kept after one dropped; the order
of the entries rotates from one run to the next, and every timed entry follows a 1 GiB read-only pass.
Runnable alone:  python bench_mixing.py [--cases halo4_f64,...] [--out PATH]
                 -> one JSON line, also written to PATH (default profiles/mixing/bench_mixing.json).
"""
import json
import os
import statistics
import sys

from bench_common import HBM_PEAK_GBPS, NX, NY, NZ, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DROP, KEPT = 1, 5
SIZE = (NX, NY, NZ)
OUT = os.path.join(ROOT, "profiles", "mixing", "bench_mixing.json")
CA = (1e-4, 0.1, 1e-2, 0.1)                                         # background kappa, convective kappa, background nu, convective nu
RI = (0.7, 0.5, 1.7, 0.1, 0.4, 0.6)                                # nu0, kappa0, kappa_ca, Ri0, Ri_delta, Cav
NAMES = ("kappa_c", "nu_c", "kappa_u", "kappa_v")


def torch_rule(torch, kind, b, u, v, prev, dz, q, size, halo):
    """the rule of csrc/staged/tripolar_hip_mixing.h as torch passes: nu_c and kappa on the interior extended by the column west and the
    row south, then the two half-sums -> the four (Nz - 1, Ny, Nx) arrays of the faces 2..Nz"""
    (nx, ny, nz), (hx, hy, hz) = size, halo
    ext = lambda a, di=0, dj=0: a[hz:hz + nz, hy - 1 + dj:hy + ny + dj, hx - 1 + di:hx + nx + di]                              # noqa: E731
    dk = lambda a, di=0, dj=0: (ext(a, di, dj)[1:] - ext(a, di, dj)[:-1]) / dz                                                # noqa: E731
    N2 = dk(b)
    if kind == "ca":
        stable = N2 >= 0
        full = lambda x: torch.full_like(N2, x)                    # noqa: E731
        kappa, nu = torch.where(stable, full(q[0]), full(q[1])), torch.where(stable, full(q[2]), full(q[3]))
    else:
        du0, du1, dv0, dv1 = dk(u), dk(u, di=1), dk(v), dk(v, dj=1)
        S2 = 0.5 * (du0 * du0 + du1 * du1) + 0.5 * (dv0 * dv0 + dv1 * dv1)
        zero, one = torch.zeros_like(N2), torch.ones_like(N2)
        Ri = torch.where(N2 == 0, zero, N2 / S2)
        x = (Ri - q[3]) / torch.full_like(N2, q[4])              # a tensor divisor: torch multiplies by the reciprocal of a number
        y = torch.where(x > 0, x, zero)
        tau = one - torch.where(y < one, y, one)
        nu, kappa = q[0] * tau, q[1] * tau
        kappa = torch.where(N2 < 0, kappa + q[2], kappa)
        if prev is not None:
            faces = lambda a: a[hz + 1:hz + nz, hy - 1:hy + ny, hx - 1:hx + nx]                                              # noqa: E731
            den = torch.ones_like(N2) + torch.full_like(N2, q[5])  # one + T(Cav), in T; a tensor divisor as above
            nu, kappa = (q[5] * faces(prev[1]) + nu) / den, (q[5] * faces(prev[0]) + kappa) / den
    own = nu[:, 1:, 1:]
    return kappa[:, 1:, 1:], own, 0.5 * (nu[:, 1:, :-1] + own), 0.5 * (nu[:, :-1, 1:] + own)


def run_case(torch, _lib, M, dev, size, h, tdt):
    halo = (h, h, h)
    (nx, ny, nz), (hx, hy, hz) = size, halo
    esz = 8 if tdt == torch.float64 else 4
    cells_shape, faces_shape = (nz + 2 * hz, ny + 2 * hy, nx + 2 * hx), (nz + 1 + 2 * hz, ny + 2 * hy, nx + 2 * hx)
    gen = torch.Generator(device=dev).manual_seed(7)
    rand = lambda s, lo, hi: torch.empty(s, dtype=tdt, device=dev).uniform_(lo, hi, generator=gen)                              # noqa: E731
    b, u, v = (rand(cells_shape, -1, 1) for _ in range(3))
    prev = (rand(faces_shape, 0, 2), rand(faces_shape, 0, 2))
    outs = [torch.zeros(faces_shape, dtype=tdt, device=dev) for _ in NAMES]
    dz_f = rand(nz + 1, 0.5, 2)
    dz = dz_f[1:nz].reshape(-1, 1, 1)
    ft = _lib.ft_of(tdt)
    lib = M.mixing_lib()
    ptr = lambda t: None if t is None else t.data_ptr()                                                                         # noqa: E731
    tail = (ptr(dz_f), None, None, None, 0.0, *size, *halo, ft)

    def ca():
        M.check_mixing(lib.tpg_convective_adjustment_diffusivities(ptr(b), *(ptr(o) for o in outs), *CA, *tail, _lib.current_stream_ptr(dev)))

    def ri(averaged):
        old = prev if averaged else (None, None)
        return lambda: M.check_mixing(lib.tpg_ri_based_diffusivities(ptr(b), ptr(u), ptr(v), ptr(old[0]), ptr(old[1]), *(ptr(o) for o in outs), *RI,
                                                                     *tail, _lib.current_stream_ptr(dev)))

    fns = {"ca_ms": ca, "ri_ms": ri(False), "ri_prev_ms": ri(True),
           "torch_ca_ms": lambda: torch_rule(torch, "ca", b, None, None, None, dz, CA, size, halo),
           "torch_ri_ms": lambda: torch_rule(torch, "ri", b, u, v, None, dz, RI, size, halo),
           "torch_ri_prev_ms": lambda: torch_rule(torch, "ri", b, u, v, prev, dz, RI, size, halo)}
    # identical bits before anything is timed: the evaluated faces of all four outputs, integer views
    ints = lambda t: t.contiguous().view(torch.int64 if esz == 8 else torch.int32)                                              # noqa: E731
    res = {"size": list(size), "halo": list(halo), "eltype": "Float64" if esz == 8 else "Float32"}
    for call, rule in (("ca_ms", "torch_ca_ms"), ("ri_ms", "torch_ri_ms"), ("ri_prev_ms", "torch_ri_prev_ms")):
        fns[call]()
        want = fns[rule]()
        torch.cuda.synchronize()
        for name, o, w in zip(NAMES, outs, want):
            got = o[hz + 1:hz + nz, hy:hy + ny, hx:hx + nx]
            assert torch.equal(ints(got), ints(w)), f"{call}: {name} differs from the torch passes"
        del want
    res["identical_bits_to_torch_passes"] = True
    res["convective_share"] = float((outs[0][hz + 1:hz + nz, hy:hy + ny, hx:hx + nx] > RI[1]).double().mean())
    cells = nx * ny * nz
    for streams in (5, 7, 9):
        half = streams * cells // 2
        pair = (rand(half, -1, 1), torch.empty(half, dtype=tdt, device=dev))
        fns[f"copy{streams}_ms"] = lambda pair=pair: pair[1].copy_(pair[0])
    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)          # 1 GiB: evicts L2 + Infinity Cache

    def once(f):
        flush.sum()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    names = list(fns)
    samples = {name: [] for name in names}
    for r in range(KEPT + DROP):
        for name in names[r % len(names):] + names[:r % len(names)]:           # the order rotates: no entry keeps one predecessor
            samples[name].append(once(fns[name]))
    for name, s in samples.items():
        res[name] = statistics.median(s[DROP:])
        res[name + "_range"] = [min(s[DROP:]), max(s[DROP:])]
    res["kept_runs"] = KEPT
    res["bytes_per_stream"] = cells * esz
    for call, streams in (("ca", 5), ("ri", 7), ("ri_prev", 9)):
        res[f"{call}_streams"] = streams
        res[f"{call}_floor_ms"] = streams * cells * esz / (HBM_PEAK_GBPS * 1e9) * 1e3
        res[f"{call}_over_copy{streams}_time"] = res[f"{call}_ms"] / res[f"copy{streams}_ms"]
        res[f"torch_{call}_over_{call}_time"] = res[f"torch_{call}_ms"] / res[f"{call}_ms"]
    res["ri_prev_over_ri_time"] = res["ri_prev_ms"] / res["ri_ms"]
    del b, u, v, prev, outs, flush
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def bench_mixing(torch, _lib, M, dev, cases=None):
    out = {}
    for tdt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"halo4_{tag}"
        if cases is None or name in cases:
            out[name] = run_case(torch, _lib, M, dev, SIZE, 4, tdt)
    out["method"] = (f"median of {KEPT} runs kept after {DROP} dropped, the order of the entries rotating, each entry after a 1 GiB read-only pass; "
                     "stream-event bracket around the call; copyN = dst.copy_(src) on contiguous tensors of half the bytes of N streams of the "
                     "interior; floor = N streams / 8 TB/s; *_range = the least and the greatest of the kept samples; torch_* = the rule as "
                     "shifted-slice torch passes, bits asserted identical first")
    return out


def main():
    import torch
    from orthogonalsphericalshellgrids.jl_amd import _lib
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    arg = lambda flag: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None                                        # noqa: E731
    cases = arg("--cases").split(",") if arg("--cases") else None
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    out = bench_mixing(torch, _lib, M, dev, cases)
    out["mixing_library"] = os.path.relpath(M.MIXING_LIB_PATH, ROOT)
    line = json.dumps(out)
    path = os.path.abspath(arg("--out")) if arg("--out") else OUT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
