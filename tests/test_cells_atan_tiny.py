"""The first atan tier of k_cells_tile (csrc/tpg_grid.hip, csrc/tpg_batch.hpp; profiles/cells_atan_tiny/README.md): for +0 <= t < 2^-14
the last Horner step of each chain of atan_small_b<N, true> is the identity, so tpgb::atan_tiny_b<N> leaves the eight fma in front of them
out -- and must give the bits of atan_small_b<N, true> everywhere below 2^-14 and report everything else as `rare`.

CPU: tpg_batch.hpp compiled for the host behind a small HIP stub (the harness of tests/test_cells_trims3.py, restated), no contraction --
  * the evaluation of atan_tiny_b<4> and <1> against the evaluation of atan_small_b<N, true>, bit for bit: +0, subnormals, the neighbours
    of 2^-27, 10^6 seeded random bit patterns in [+0, 2^-14), the last 10^5 doubles below 2^-14, every power of two from 2^-1074 to 2^-15
    with its +-1 ulp neighbours;
  * at 2^-14, its upper neighbour, -0.0, negatives, NaN and +-Inf the helper reports `rare`, and the three-tier caller of the kernel
    (tiny, then atan_small_b<4, true>, then atan_b<4>) gives the bits of the two-tier caller it replaces, groups of 4 with a single
    non-tiny element included; at least 10^6 arguments take the tiny form and at least 10^3 each other tier.
GPU: the probe's B_ATAN_TINY against the scalar atanD on the device; all 20 whole padded arrays of tpg_build_grid against the oracle and
against the thread-per-cell kernel (TPG_CELLS_VARIANT=0 of the test library), bit for bit, at 480 x 240 (every wave on the tiny form; both
tile orders; fplp90 = 45, 160.3, 190.7, 380), 400 x 200 (the threshold is crossed inside rows), 360 x 180 (a third of the cells on the
middle tier), 60 x 30 and 124 x 21 (no wave tiny), Float32 at 482 x 240, and one 15-row band of 1440 x 720 with jstart > Hy + 1 against
the same rows of the oracle's global arrays.  What a shape is there for is asserted from the oracle's Az / (4 R^2), the size of a
half-cell triangle's tangent, before the comparison.  3600 x 1800 is tests/test_gpu_grid.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
TINY = 2.0 ** -14

# ---- CPU: the helper against the form it shortens ----------------------------------------------------------------------------------
# what the two headers need of the HIP device environment, for a host compiler
_HIP_STUB = r"""
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#define __noinline__ __attribute__((noinline))
static inline int __double2hiint(double x) { int64_t u; std::memcpy(&u, &x, 8); return (int)(u >> 32); }
static inline int __double2loint(double x) { int64_t u; std::memcpy(&u, &x, 8); return (int)(u & 0xffffffff); }
static inline double __hiloint2double(int hi, int lo) { uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo; double x; std::memcpy(&x, &u, 8); return x; }
static inline long long __double_as_longlong(double x) { long long u; std::memcpy(&u, &x, 8); return u; }
static inline double __longlong_as_double(long long u) { double x; std::memcpy(&x, &u, 8); return x; }
static inline double __builtin_amdgcn_rcp(double x) { return 1.0 / x; }
static inline double __builtin_amdgcn_rsq(double x) { return 1.0 / std::sqrt(x); }
static inline unsigned __builtin_amdgcn_ubfe(unsigned v, unsigned off, unsigned w) { return (v >> off) & ((1u << w) - 1u); }
static inline bool __any(bool p) { return p; }
using std::fmod; using std::sqrt;
"""

_HARNESS = r"""
#include "tpg_batch.hpp"

extern "C" {
// out[0]: atan_tiny_b<4>; [1]: atan_small_b<4, true>; [2], [3]: the same as one-element batches.  rare[0..3]: what each reported.
void atan_tiny_forms(const double* x, long n, double* out, int* rare)
{
    for (long i = 0; i + 3 < n; i += 4) {
        double a[4] = { x[i], x[i + 1], x[i + 2], x[i + 3] }, o[4];
        const bool rt = tpgb::atan_tiny_b<4>(a, o);
        for (int e = 0; e < 4; ++e) { out[i + e] = o[e]; rare[i + e] = rt; }
        const bool rs = tpgb::atan_small_b<4, true>(a, o);
        for (int e = 0; e < 4; ++e) { out[n + i + e] = o[e]; rare[n + i + e] = rs; }
    }
    for (long i = 0; i < n; ++i) {
        double a[1] = { x[i] }, o[1];
        rare[2 * n + i] = tpgb::atan_tiny_b<1>(a, o); out[2 * n + i] = o[0];
        rare[3 * n + i] = tpgb::atan_small_b<1, true>(a, o); out[3 * n + i] = o[0];
    }
}
// the kernel's caller around a batch of 4 tangents, now (out[0], tier[0]: 0 tiny, 1 the full polynomial, 2 the fallback) and as it was
// (out[1], tier[1]: 1 or 2).  The fallback of the kernel forms its tangents again with IEEE division; here the argument is the tangent.
void atan_callers(const double* x, long n, double* out, int* tier)
{
    for (long i = 0; i + 3 < n; i += 4) {
        double a[4] = { x[i], x[i + 1], x[i + 2], x[i + 3] }, at[4];
        int t = 0;
        if (__any(tpgb::atan_tiny_b<4>(a, at))) {
            t = 1;
            if (__any(tpgb::atan_small_b<4, true>(a, at))) { t = 2; tpgb::atan_b<4>(a, at); }
        }
        for (int e = 0; e < 4; ++e) { out[i + e] = at[e]; tier[i + e] = t; }
        t = 1;
        if (__any(tpgb::atan_small_b<4, true>(a, at))) { t = 2; tpgb::atan_b<4>(a, at); }
        for (int e = 0; e < 4; ++e) { out[n + i + e] = at[e]; tier[n + i + e] = t; }
    }
}
}
"""


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """atan_tiny_b, atan_small_b and atan_b of csrc/tpg_batch.hpp compiled for the host (no contraction, as csrc/Makefile)"""
    d = tmp_path_factory.mktemp("atan_tiny")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(_HIP_STUB)
    (d / "harness.cpp").write_text(_HARNESS)
    so = d / "libatantiny.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wno-unknown-pragmas",
                        "-Wno-attributes", "-I", str(d), "-I", CSRC, "-o", str(so), str(d / "harness.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    for name in ("atan_tiny_forms", "atan_callers"):
        getattr(lib, name).argtypes = [dp, C.c_long, dp, ip]
        getattr(lib, name).restype = None
    return lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    """bit for bit; two NaNs count as the same result"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


TINY_BITS = int(_bits(np.array([TINY]))[0])                                      # 0x3F10000000000000


def _pad4(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([x, np.full((-x.size) % 4, x[-1])]))


def _tiny_sets():
    """the argument sets of the tiny form, all in [+0, 2^-14)"""
    rng = np.random.default_rng(20261020)
    sub = np.concatenate([[5e-324, 1e-310, 2.2250738585072009e-308, 2.2250738585072014e-308], _from_bits(rng.integers(1, 1 << 52, 1000))])
    p27 = np.array([2.0 ** -27, np.nextafter(2.0 ** -27, 0.0), np.nextafter(2.0 ** -27, 1.0)])
    rnd = _from_bits(rng.integers(0, TINY_BITS, 1_000_000))
    last = _from_bits(TINY_BITS - np.arange(1, 100_001, dtype=np.uint64))
    p2 = np.ldexp(1.0, np.arange(-1074, -14))
    pows = np.concatenate([p2, np.nextafter(p2, 0.0), np.nextafter(p2, 1.0)])
    x = np.concatenate([[0.0], sub, p27, rnd, last, pows])
    assert ((x >= 0) & ~np.signbit(x) & (x < TINY)).all() and p2[0] == 5e-324 and p2[-1] == 2.0 ** -15
    return x


def _threshold_values():
    """what the helper must report as rare: 2^-14, its upper neighbour, -0.0, negatives, NaN, +-Inf (and what lies above)"""
    return np.array([TINY, np.nextafter(TINY, 1.0), -0.0, -5e-324, -1e-300, -2.0 ** -27, -1e-6, -TINY, -0.3, -1.0, -1e300, np.nan, np.inf, -np.inf,
                     2.0 ** -13, 1e-3, 0.4375, np.nextafter(0.4375, 0.0), np.nextafter(0.4375, 1.0), 1.0, 1e300])


def test_tiny_form_equals_the_full_polynomial_below_two_to_the_minus_14(forms):
    x = _pad4(_tiny_sets())
    out, rare = np.zeros((4, x.size)), np.ones((4, x.size), dtype=np.int32)
    forms.atan_tiny_forms(x, x.size, out, rare)
    assert x.size >= 1_000_000 and not rare.any()                                # in the domain of both forms, batches of 4 and of 1
    for tiny, small, what in ((0, 1, "N = 4"), (2, 3, "N = 1")):
        bad = np.flatnonzero(_bits(out[tiny]) != _bits(out[small]))
        assert bad.size == 0, (what, bad.size, x[bad[:5]].tolist(), out[tiny][bad[:5]].tolist(), out[small][bad[:5]].tolist())
    assert np.array_equal(_bits(out[0]), _bits(out[2]))
    assert not np.signbit(out[0]).any() and _bits(out[0][:1])[0] == 0            # +0 -> +0


def test_helper_reports_everything_outside_its_domain(forms):
    v = _threshold_values()
    x = _pad4(np.concatenate([v, np.repeat(1e-6, 4)]))
    out, rare = np.zeros((4, x.size)), np.zeros((4, x.size), dtype=np.int32)
    forms.atan_tiny_forms(x, x.size, out, rare)
    assert rare[2][:v.size].all() and not rare[2][v.size:].any()                 # one-element batches: each value by itself
    ok = (x >= 0) & ~np.signbit(x) & (x < TINY)
    assert np.array_equal(rare[2] == 0, ok)
    assert np.array_equal(rare[0] == 0, ok.reshape(-1, 4).all(axis=1).repeat(4))  # batches of 4: the OR over the elements


def test_three_tier_caller_gives_the_bits_of_the_two_tier_caller(forms):
    rng = np.random.default_rng(14)
    tiny = _pad4(_tiny_sets())
    v = _threshold_values()
    # groups of 4 with a single element outside the tiny domain, at each position, among tiny elements of the kernel's size
    mixed = np.full((v.size * 4, 4), 1.3e-6)
    for k, val in enumerate(np.repeat(v, 4)):
        mixed[k, k % 4] = val
    middle = rng.uniform(TINY, 0.4375, 4000)                                     # whole groups on the full polynomial
    middle[:2] = [TINY, np.nextafter(0.4375, 0.0)]
    beyond = np.concatenate([rng.uniform(0.4375, 5.0, 1500), -rng.uniform(0.0, 5.0, 1500), 10.0 ** rng.uniform(1, 300, 500), -10.0 ** rng.uniform(-300, -5, 500)])
    x = np.concatenate([tiny, mixed.ravel(), _pad4(v), middle, beyond])
    assert x.size % 4 == 0
    out, tier = np.zeros((2, x.size)), np.full((2, x.size), -1, dtype=np.int32)
    forms.atan_callers(x, x.size, out, tier)
    bad = np.flatnonzero(~_same(out[0], out[1]))
    assert bad.size == 0, (bad.size, x[bad[:5]].tolist(), out[0][bad[:5]].tolist(), out[1][bad[:5]].tolist(), tier[0][bad[:5]].tolist())
    # the tiers are the ones claimed: tiny <=> the whole group in [+0, 2^-14); what took the fallback before takes it now and nothing else does
    grp = lambda m: m.reshape(-1, 4).all(axis=1).repeat(4)                       # noqa: E731
    pos = (x >= 0) & ~np.signbit(x)
    assert np.array_equal(tier[0] == 0, grp(pos & (x < TINY)))
    assert np.array_equal(tier[0] == 2, tier[1] == 2) and np.array_equal(tier[0] == 2, ~grp(pos & (x < 0.4375)))
    assert set(np.unique(tier[0])) == {0, 1, 2} and set(np.unique(tier[1])) == {1, 2}
    counts = [int((tier[0] == t).sum()) for t in range(3)]
    assert counts[0] >= 1_000_000 and counts[1] >= 1000 and counts[2] >= 1000, counts
    single = tier[0][tiny.size:tiny.size + mixed.size].reshape(-1, 4)[:, 0]      # every mixed group left the tiny form, to the tier its one element needs
    want = np.where((np.repeat(v, 4) >= 0) & ~np.signbit(np.repeat(v, 4)) & (np.repeat(v, 4) < 0.4375), 1, 2)
    assert np.array_equal(single, want)


# ---- GPU: the helper in place, and every tier of the kernel on whole padded arrays -------------------------------------------------
B_ATAN_TINY, F_ATAN = 111, 5                                                     # csrc/tpg_probe.hip


@pytest.mark.gpu
def test_device_helper_equals_the_scalar_atan_and_flags_the_rest(gpu):
    import torch
    from tools import testlib
    lib = testlib.lib()
    tiny = _tiny_sets()
    rng = np.random.default_rng(3)
    x = np.concatenate([_pad4(tiny[rng.choice(tiny.size, 200_000, replace=False)]), _pad4(tiny[-3300:]), np.repeat(_threshold_values(), 4)])
    xd = torch.from_numpy(x).to(gpu)
    res = []
    for which in (B_ATAN_TINY, F_ATAN):
        yd, rd = torch.empty_like(xd), torch.zeros(xd.numel(), dtype=torch.int32, device=gpu)
        assert lib.tpg_math_probe(which, xd.data_ptr(), yd.data_ptr(), rd.data_ptr(), xd.numel(), None) == 0
        torch.cuda.synchronize()
        res.append((yd.cpu().numpy(), rd.cpu().numpy() != 0))
    (y, rare), (want, _) = res
    ok = (x >= 0) & ~np.signbit(x) & (x < TINY)
    assert np.array_equal(~rare, ok) and ok.sum() > 200_000 and (~ok).sum() >= 80
    bad = np.flatnonzero(ok & (_bits(y) != _bits(want)))
    assert bad.size == 0, (bad.size, x[bad[:5]].tolist(), y[bad[:5]].tolist(), want[bad[:5]].tolist())


H4 = (4, 4, 4)
# (size, extra keywords, float32?, (ranks, rank) of a latitude band or None, TPG_CELLS_ORDER or None = the product's)
CASES = [((480, 240, 1), {}, False, None, order) for order in (0, 1)]            # every wave on the tiny form; 8 x 35 tiles, both orders
CASES += [((400, 200, 1), {}, False, None, None)]                                # the threshold is crossed inside rows
CASES += [((360, 180, 1), {}, False, None, None)]                                # a third of the cells on the full polynomial
CASES += [((60, 30, 1), {}, False, None, None), ((124, 21, 1), {}, False, None, None)]   # no wave tiny
# fplp90 = 45, 160.3, 190.7 | 380: beyond 360 the whole grid takes the general path
CASES += [((480, 240, 1), dict(first_pole_longitude=fpl), False, None, None) for fpl in (-45.0, 70.3, 100.7, 290.0)]
CASES += [((482, 240, 1), {}, True, None, None)]                                 # Float32, Nx = 2 (mod 4)
CASES += [((1440, 720, 1), {}, False, (48, 30), None)]                           # rows 451 .. 465: jstart > Hy + 1, an ordinary apron row
# what the share of the interior cells whose Az / (4 R^2) lies below 2^-14 must be, by shape
PREMISE = {(480, 240): "all", (482, 240): "all", (1440, 720): "all", (400, 200): "part", (360, 180): "part", (60, 30): "few", (124, 21): "few"}
PREMISE_HOLDS = {"all": lambda s: s == 1.0, "part": lambda s: 0.5 < s < 0.995, "few": lambda s: s < 0.01}


def _id(case):
    size, kw, f32, band, order = case
    return (f"{size[0]}x{size[1]}" + ("-f32" if f32 else "") + (f"-fpl{kw['first_pole_longitude']}" if kw else "")
            + (f"-band{band[1]}of{band[0]}" if band else "") + ("" if order is None else f"-order{order}"))


_ref = {}


def _arrays(osg, case):
    import torch
    size, kw, f32, band, _ = case
    arch = osg.GPU(0) if band is None else osg.Distributed(osg.GPU(0), osg.Partition(y=band[0]), local_rank=band[1])
    g = osg.TripolarGrid(arch, torch.float32 if f32 else torch.float64, size=size, halo=H4, **kw)
    return {n: getattr(g, n).cpu().numpy() for n in osg._lib.ARRAY_NAMES}, (g.jrange if band else None)


def _band_rows(case):
    size, _, _, band, _ = case
    ny = size[1] // band[0]
    return band[1] * ny + 1, band[1] * ny + ny


def _reference(oracle, case):
    """the oracle's arrays of a case: computed once, shared by the tile orders and the two tests, left unchanged.  The premise of the
    shape is asserted on the way.  A band is cut out of the oracle's GLOBAL arrays: its rows jstart - Hy .. jend + Hy."""
    size, kw, f32, band, _ = case
    key = _id(case[:4] + (None,))
    if key not in _ref:
        ref = oracle.build_grid(size, dtype=np.float32 if f32 else np.float64, halo=H4, **kw)
        Hx, Hy = H4[0], H4[1]
        j0, j1 = _band_rows(case) if band else (1, size[1])
        tan = np.concatenate([ref[n][Hy + j0 - 1:Hy + j1, Hx:Hx + size[0]].astype(np.float64).ravel() for n in ("az_cc", "az_ff")]) / (4.0 * oracle.R_EARTH ** 2)
        assert np.isfinite(tan).all() and (tan > 0).all()
        share = float((tan < TINY).mean())
        assert PREMISE_HOLDS[PREMISE[size[:2]]](share), (key, PREMISE[size[:2]], share, float(tan.max()))
        if band:
            ref = {n: np.ascontiguousarray(a[j0 - 1:j1 + 2 * Hy]) for n, a in ref.items()}
        for a in ref.values():
            a.setflags(write=False)
        _ref[key] = ref
    return _ref[key]


def _assert_same(got, want, what):
    assert len(want) == 20 and set(got) == set(want)
    for name, r in want.items():
        a = got[name]
        assert a.shape == r.shape and a.dtype == r.dtype, (what, name)
        same = _bits(a) == _bits(r)
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def test_cases_are_the_ones_each_tier_needs():
    sizes = [c[0][:2] for c in CASES]
    assert {(480, 240), (400, 200), (360, 180), (60, 30), (124, 21), (482, 240), (1440, 720)} == set(sizes) and set(sizes) == set(PREMISE)
    assert {c[4] for c in CASES if c[0][:2] == (480, 240) and not c[1]} == {0, 1}
    assert {c[1]["first_pole_longitude"] + 90.0 for c in CASES if c[1]} == {45.0, 160.3, 190.7, 380.0} and all(c[0][:2] == (480, 240) for c in CASES if c[1])
    assert [c[0][:2] for c in CASES if c[2]] == [(482, 240)]
    bands = [c for c in CASES if c[3]]
    assert len(bands) == 1 and _band_rows(bands[0]) == (451, 465) and _band_rows(bands[0])[0] > H4[1] + 1


@pytest.fixture
def knobs(osg, via_testlib):
    """TPG_CELLS_VARIANT / TPG_CELLS_ORDER of the test library, restored afterwards"""
    names = ("TPG_CELLS_VARIANT", "TPG_CELLS_ORDER")
    saved = {n: os.environ.get(n) for n in names}

    def select(**kw):
        for n in names:
            v = kw.get(n)
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = str(v)
        via_testlib.tpg_reload_config()
    yield select
    for n, v in saved.items():
        if v is None:
            os.environ.pop(n, None)
        else:
            os.environ[n] = v
    via_testlib.tpg_reload_config()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_twenty_arrays_equal_the_oracle_bit_for_bit(osg, oracle, gpu, knobs, case):
    want = _reference(oracle, case)
    knobs(TPG_CELLS_VARIANT=2, TPG_CELLS_ORDER=case[4])
    got, jrange = _arrays(osg, case)
    if case[3]:
        assert tuple(jrange) == _band_rows(case)
    _assert_same(got, want, "oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tile_kernel_equals_the_thread_per_cell_kernel(osg, gpu, knobs, case):
    knobs(TPG_CELLS_VARIANT=0)
    want, _ = _arrays(osg, case)
    knobs(TPG_CELLS_VARIANT=2, TPG_CELLS_ORDER=case[4])
    got, _ = _arrays(osg, case)
    _assert_same(got, want, "thread per cell")
