"""The seedless divisions of k_cells_tile (csrc/tpg_math.hpp, csrc/tpg_batch.hpp, csrc/tpg_grid.hip; profiles/cells_seedless/README.md):
for a denominator b = (1 - d) / c next to a known constant, c = 1 (the asin tail of a haversine) or c = 1/4 (the four triangle
denominators of a quadrilateral), tpgm::div_near runs div_nr's seven operations from r = c instead of v_rcp_f64(b) -- and must give the
bits of div_nr, which are those of IEEE a / b, wherever a caller's tier test lets it run.

CPU: tpg_math.hpp and tpg_batch.hpp compiled for the host behind a small HIP stub (the harness of tests/test_cells_atan_tiny.py,
restated), no contraction --
  * both forms against IEEE `/` and against the host evaluation of div_nr, bit for bit: 10^7 seeded random pairs per form over the whole
    domain of the helper (d of both signs, 2^-46 <= |d| < 2^-14, numerators of both signs over 60 binades), every power of two of d from
    2^-1074 to 2^-15 with its +-1 ulp neighbours in both signs (b = RN((1 - d) / c): below 2^-54 that is b = 1 / c itself), the last 10^5
    doubles below each threshold (2^-16 of the tier test, 2^-14 of the helper), b = 1 / c and one and two ulps above it, a = +0.
    a = -0 is outside the callers' domain (their numerators are |x| or t p(t), t > 0) and gives +0 where IEEE gives -0, through div_nr
    just the same: held against div_nr only.  Subnormal quotients are outside the callers' domain as they are outside div_nr's (a = 0 or a / b comfortably normal) and are not sent;
  * `rare` of div_near_b at 2^-16 and its upper neighbour, d < 0, NaN, +-Inf, b far from 1 / c; the tier of asin_sqrt_b at r = 2^-8, its
    neighbours, NaN, -Inf, negative h, h = +-0;
  * the tiered callers against the forms they replace (asin_sqrt_b against its two-tier form restated here and against the scalar
    asinD(min(sqrt(h), 1)); the four-tangent group of phase 2 against tri_tan_nr + the three atan tiers), exactly one non-tiny element at
    each position of a batch included; the tier of every group checked and counted (>= 10^6 tiny, >= 10^3 each other tier).
GPU: the probe's B_DIV_NEAR1 / B_DIV_NEAR4 against the device's div_nr (F_DIV_NR) on the CPU test's edge set; all 20 whole padded arrays
of tpg_build_grid against the oracle and against the thread-per-cell kernel (TPG_CELLS_VARIANT=0 of the test library), bit for bit, in
both tile orders: rows 451-465 of 1440 x 720 and rows 1-15 of 3600 x 1800 as bands (every wave on the seedless form of both sites), rows
1786-1800 of 3600 x 1800 (row Ny: fold, substitution and pole-adjacent cells beside the tiny tier), 800 x 400 (mixed), 480 x 240 and
60 x 30 (the forms of before), Float32 at 482 x 240.  What a shape is there for is asserted from the oracle's edge lengths before the
comparison: per block of 30 columns of a row -- the strip of a cell wave; its second strip holds the lambda -> -lambda images, which have
the same sizes -- r = sin(d / 2R) of the longest of the eight edges against 2^-8, and (dx^2 + dy^2) / (4 R^2), the size of a half-cell
triangle's d, against 2^-16.
Two departures from the shapes first planned, both read from the oracle: 720 x 360 has 9.1 % of its cell waves on the seedless
triangle form, under the 10 % asked of a mixed shape, so the mixed shape is 800 x 400 (17 % / 83 % at the triangles, 88 % / 12 % at the
haversines); and 480 x 240 is not on the second tier THROUGHOUT -- the cells next to the two northern poles are small on any grid -- but
with 94 % / 91 % of its waves: asserted as "most"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
D_TIER, D_HELPER, R_TINY = 2.0 ** -16, 2.0 ** -14, 2.0 ** -8

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
using namespace tpgm;

// asin_sqrt_b as it was before the seedless tier: its two-tier form, restated
template <int N> static bool asin_sqrt_before(const double (&h)[N], double (&out)[N])
{
    double rt[N];
    bool rare = false;
    for (int e = 0; e < N; ++e) { rt[e] = sqrt_nr<true>(h[e]); rare |= !(rt[e] < 0.5); }
    tpgb::asin_small_poly_b<N>(rt, out);
    if (rare)
        for (int e = 0; e < N; ++e) { const double r = sqrt_nr(h[e]); out[e] = asinD(!(r >= 1.0) ? r : 1.0); }
    return rare;
}
template <int N> static void asin_groups(const double* h, long n, double* out, int* tier)
{
    for (long i = 0; i + N - 1 < n; i += N) {
        double a[N], o[N];
        for (int e = 0; e < N; ++e) a[e] = h[i + e];
        int t = -1;
        const bool ran = tpgb::asin_sqrt_b<N>(a, o, &t);
        if (ran != (t == 2)) t = -2;
        for (int e = 0; e < N; ++e) { out[i + e] = o[e]; tier[i + e] = t; }
        const bool r = asin_sqrt_before<N>(a, o);
        for (int e = 0; e < N; ++e) { out[n + i + e] = o[e]; tier[n + i + e] = r ? 2 : 1; }
    }
}

extern "C" {
// out[0]: div_near; [1]: div_nr; [2]: IEEE a / b
void div_forms(const double* a, const double* b, long n, int quarter, double* out)
{
    for (long i = 0; i < n; ++i) {
        out[i] = quarter ? div_near<true>(a[i], b[i]) : div_near<false>(a[i], b[i]);
        out[n + i] = div_nr(a[i], b[i]);
        out[2 * n + i] = a[i] / b[i];
    }
}
// what div_near_b reports, element by element (one-element batches) and for groups of 4
void div_rare(const double* b, long n, int quarter, int* rare)
{
    for (long i = 0; i < n; ++i) {
        const double a1[1] = { 1.0 }, b1[1] = { b[i] };
        double o1[1];
        rare[i] = quarter ? tpgb::div_near_b<1, true>(a1, b1, o1) : tpgb::div_near_b<1, false>(a1, b1, o1);
    }
    for (long i = 0; i + 3 < n; i += 4) {
        const double a4[4] = { 1.0, 1.0, 1.0, 1.0 }, b4[4] = { b[i], b[i + 1], b[i + 2], b[i + 3] };
        double o4[4];
        const bool r = quarter ? tpgb::div_near_b<4, true>(a4, b4, o4) : tpgb::div_near_b<4, false>(a4, b4, o4);
        for (int e = 0; e < 4; ++e) rare[n + i + e] = r;
    }
}
// asin_sqrt_b now (out[0], tier[0]: 0 seedless, 1 the polynomial with div_nr, 2 the scalar fallback ran) and before (out[1], tier[1]),
// in the kernel's batches of 2 and of 1; out[2]: the scalar asinD(min(sqrt(h), 1)) with IEEE sqrt, as the reference has it
void asin_callers(const double* h, long n, int batch, double* out, int* tier)
{
    if (batch == 2) asin_groups<2>(h, n, out, tier); else asin_groups<1>(h, n, out, tier);
    for (long i = 0; i < n; ++i) { const double r = std::sqrt(h[i]); out[2 * n + i] = asinD(!(r >= 1.0) ? r : 1.0); }
}
// phase 2's four tangents of a quadrilateral and their atans: now (out[0] tangents, out[2] atans; tier[0]: 0 seedless, 1 div_nr;
// tier[2]: the atan tier) and as they were (out[1], out[3]; tier[1] = 1, tier[3]).  The last atan tier of the kernel forms its tangents
// again with IEEE division; so does this.
void tan_callers(const double* num, const double* den, long n, double* out, int* tier)
{
    for (long i = 0; i + 3 < n; i += 4) {
        double tn[4], td[4], tt[4], at[4];
        for (int e = 0; e < 4; ++e) { tn[e] = num[i + e]; td[e] = den[i + e]; }
        for (int form = 0; form < 2; ++form) {
            int t = 1, ta = 0;
            if (form == 0) {
                t = 0;
                if (__any(tpgb::div_near_b<4, true>(tn, td, tt))) { t = 1; for (int e = 0; e < 4; ++e) tt[e] = div_nr(tn[e], td[e]); }
            } else {
                for (int e = 0; e < 4; ++e) tt[e] = div_nr(tn[e], td[e]);
            }
            for (int e = 0; e < 4; ++e) out[form * n + i + e] = tt[e];
            if (__any(tpgb::atan_tiny_b<4>(tt, at))) {
                ta = 1;
                if (__any(tpgb::atan_small_b<4, true>(tt, at))) { ta = 2; for (int e = 0; e < 4; ++e) tt[e] = tn[e] / td[e]; tpgb::atan_b<4>(tt, at); }
            }
            for (int e = 0; e < 4; ++e) { out[(2 + form) * n + i + e] = at[e]; tier[form * n + i + e] = t; tier[(2 + form) * n + i + e] = ta; }
        }
    }
}
}
"""


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """div_near, div_near_b, asin_sqrt_b and the atan tiers of csrc/ compiled for the host (no contraction, as csrc/Makefile)"""
    d = tmp_path_factory.mktemp("seedless")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(_HIP_STUB)
    (d / "harness.cpp").write_text(_HARNESS)
    so = d / "libseedless.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wno-unknown-pragmas",
                        "-Wno-attributes", "-I", str(d), "-I", CSRC, "-o", str(so), str(d / "harness.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.div_forms.argtypes = [dp, dp, C.c_long, C.c_int, dp]
    lib.div_rare.argtypes = [dp, C.c_long, C.c_int, ip]
    lib.asin_callers.argtypes = [dp, C.c_long, C.c_int, dp, ip]
    lib.tan_callers.argtypes = [dp, dp, C.c_long, dp, ip]
    for name in ("div_forms", "div_rare", "asin_callers", "tan_callers"):
        getattr(lib, name).restype = None
    return lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    """bit for bit; two NaNs count as the same result"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


def _c(quarter):
    return 0.25 if quarter else 1.0


def _b_of(d, quarter):
    """b = RN((1 - d) / c): 1 - d rounds once, the division by a power of two is exact"""
    return (1.0 - d) / _c(quarter)


def _d_of(b, quarter):
    """the d that the tier test reads: 1 - b c, exact next to 1 / c"""
    with np.errstate(invalid="ignore", over="ignore"):
        return 1.0 - b * _c(quarter)


def _numerators(rng, n):
    return np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-30, 31, n)) * rng.choice([-1.0, 1.0], n)


def _edge_denominators(quarter):
    """the denominators of the edge set, all inside the helper's domain |d| < 2^-14"""
    p2 = np.ldexp(1.0, np.arange(-1074, -14))
    d = np.concatenate([p2, np.nextafter(p2, 0.0), np.nextafter(p2, 1.0)])
    d = np.concatenate([d, -d])
    b = [_b_of(d, quarter)]
    one = np.float64(1.0 / _c(quarter))
    b.append(np.array([one, np.nextafter(one, np.inf), np.nextafter(np.nextafter(one, np.inf), np.inf), np.nextafter(one, 0.0)]))
    for thr in (D_TIER, D_HELPER):                                                # the last 10^5 doubles with d below the threshold
        b.append(_from_bits(int(_bits(np.array([_b_of(thr, quarter)]))[0]) + np.arange(1, 100_001, dtype=np.uint64)))
    b = np.concatenate(b)
    assert (np.abs(_d_of(b, quarter)) < D_HELPER).all() and p2[0] == 5e-324 and p2[-1] == 2.0 ** -15
    return b


def _edge_pairs(quarter, seed):
    rng = np.random.default_rng(seed)
    b = _edge_denominators(quarter)
    a = _numerators(rng, b.size)
    a[::97] = 0.0
    a[1::97] = -0.0
    a[2::97] = 1.0
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _check_forms(forms, a, b, quarter, what):
    out = np.zeros((3, a.size))
    forms.div_forms(a, b, a.size, int(quarter), out)
    nz = ~((a == 0) & np.signbit(a))                                              # a = -0: outside the callers' domain, see the docstring
    for k, ref in ((2, "IEEE a / b"), (1, "div_nr")):
        bad = np.flatnonzero((_bits(out[0]) != _bits(out[k])) & (nz | (k == 1)))
        assert bad.size == 0, (what, ref, bad.size, a[bad[:5]].tolist(), b[bad[:5]].tolist(), out[0][bad[:5]].tolist(), out[k][bad[:5]].tolist())


@pytest.mark.parametrize("quarter", [False, True], ids=["c1", "c025"])
def test_seedless_division_has_the_bits_of_ieee_and_of_div_nr_on_random_pairs(forms, quarter):
    rng = np.random.default_rng(20261020 + int(quarter))
    total = 0
    for _ in range(4):                                                            # 4 x 2.5 * 10^6 pairs
        n = 2_500_000
        d = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-46, -14, n) - 1) * rng.choice([-1.0, 1.0], n)      # 2^-46 <= |d| < 2^-14
        b = np.ascontiguousarray(_b_of(d, quarter))
        assert (np.abs(_d_of(b, quarter)) < D_HELPER).all()
        _check_forms(forms, np.ascontiguousarray(_numerators(rng, n)), b, quarter, "random")
        total += n
    assert total == 10_000_000


@pytest.mark.parametrize("quarter", [False, True], ids=["c1", "c025"])
def test_seedless_division_on_the_edge_set(forms, quarter):
    a, b = _edge_pairs(quarter, 7)
    assert b.size > 200_000 and (a == 0).sum() > 4000 and np.signbit(a[a == 0]).any()
    _check_forms(forms, a, b, quarter, "edges")
    out = np.zeros((3, a.size))
    forms.div_forms(a, b, a.size, int(quarter), out)
    z = a == 0
    assert (_bits(out[0][z]) == 0).all() and np.array_equal(_bits(out[0][z]), _bits(out[1][z]))   # +0 / b = +0; -0 / b = +0 as through div_nr


def _far_denominators(quarter):
    one = 1.0 / _c(quarter)
    thr = _b_of(D_TIER, quarter)                                                  # d = 2^-16 exactly: the first rare value
    return np.array([thr, np.nextafter(thr, 0.0), np.nextafter(one, np.inf), one * (1 + 2.0 ** -30), np.nan, np.inf, -np.inf, 0.0, -0.0, -one,
                     1.0 if quarter else 4.0, 0.5 * one, 2.0 * one, 1e-300, 1e300, _b_of(D_HELPER, quarter), _b_of(2.0 ** -15, quarter)])


@pytest.mark.parametrize("quarter", [False, True], ids=["c1", "c025"])
def test_batch_form_reports_everything_outside_its_tier(forms, quarter):
    one = 1.0 / _c(quarter)
    thr = _b_of(D_TIER, quarter)
    inside = np.array([one, np.nextafter(one, 0.0), np.nextafter(thr, np.inf), _b_of(1.5e-6, quarter), _b_of(1e-5, quarter), _b_of(2.0 ** -17, quarter)])
    far = _far_denominators(quarter)
    b = np.ascontiguousarray(np.concatenate([inside, far, np.repeat(inside[3], (-(inside.size + far.size)) % 4 + 4)]))
    rare = np.zeros((2, b.size), dtype=np.int32)
    forms.div_rare(b, b.size, int(quarter), rare)
    d = _d_of(b, quarter)
    ok = (d >= 0) & (d < D_TIER)                                                  # NaN: neither
    assert ok[:inside.size].all() and not ok[inside.size:inside.size + far.size].any()
    assert np.array_equal(rare[0] == 0, ok)
    assert np.array_equal(rare[1] == 0, ok.reshape(-1, 4).all(axis=1).repeat(4))  # batches of 4: the OR over the elements


def _asin_sets(rng):
    """h of the haversine tail: the seedless tier's (sqrt(h) < 2^-8), the polynomial's, the fallback's, and what sits at the thresholds"""
    tiny = np.concatenate([10.0 ** rng.uniform(-34, np.log10(R_TINY ** 2), 1_000_000), rng.uniform(0, R_TINY ** 2, 100_000) + 1e-34,
                           _from_bits(int(_bits(np.array([R_TINY ** 2]))[0]) - np.arange(1, 100_001, dtype=np.uint64)),
                           np.array([7.6e-7, 4.76e-6, 1e-34, 1e-20])])
    assert tiny.size % 2 == 0                                                     # the groups behind it start on a batch boundary
    edge = np.array([R_TINY ** 2, np.nextafter(R_TINY ** 2, 1.0), 2.0 ** -15, 1e-3, 0.2, np.nextafter(0.25, 0.0),        # the polynomial with div_nr
                     0.25, np.nextafter(0.25, 1.0), 0.5, 0.95, 1.0, np.nextafter(1.0, 2.0), 1.5, 0.0, -0.0, -1e-300, -1e-6, -1.0, np.nan, -np.inf])
    middle = rng.uniform(R_TINY ** 2, 0.25, 4000)
    beyond = np.concatenate([rng.uniform(0.25, 1.2, 3000), np.zeros(500), -rng.uniform(0, 1, 500)])
    return tiny, edge, middle, beyond


def _asin_tier(h, batch):
    with np.errstate(invalid="ignore"):
        r = np.where(h > 0, np.sqrt(np.where(h > 0, h, 1.0)), np.nan)             # the unscaled square root of +-0, a negative h or a NaN is NaN
    r[np.isposinf(h)] = np.nan                                                    # rsq(Inf) = 0, Inf * 0
    grp = lambda m: m.reshape(-1, batch).all(axis=1).repeat(batch)                # noqa: E731
    return np.where(grp(r < R_TINY), 0, np.where(grp(r < 0.5), 1, 2))


@pytest.mark.parametrize("batch", [2, 1])
def test_asin_tail_gives_the_bits_of_its_two_tier_form(forms, batch):
    rng = np.random.default_rng(8 + batch)
    tiny, edge, middle, beyond = _asin_sets(rng)
    mixed = np.full((edge.size * 2, 2), 7.6e-7)                                   # exactly one element outside the seedless tier, at each position
    for k, val in enumerate(np.repeat(edge, 2)):
        mixed[k, k % 2] = val
    h = np.concatenate([tiny, mixed.ravel(), edge, middle, beyond])
    h = np.ascontiguousarray(np.concatenate([h, np.full(h.size % 2, 7.6e-7)]))
    out, tier = np.zeros((3, h.size)), np.full((2, h.size), -1, dtype=np.int32)
    forms.asin_callers(h, h.size, batch, out, tier)
    want = _asin_tier(h, batch)
    assert np.array_equal(tier[0], want), np.flatnonzero(tier[0] != want)[:8].tolist()
    assert np.array_equal(tier[1], np.maximum(want, 1))                           # what took the fallback before takes it now and nothing else does
    for k, ref in ((1, "two-tier form"), (2, "scalar asin")):
        bad = np.flatnonzero(~_same(out[0], out[k]))
        assert bad.size == 0, (ref, bad.size, h[bad[:5]].tolist(), out[0][bad[:5]].tolist(), out[k][bad[:5]].tolist(), tier[0][bad[:5]].tolist())
    counts = [int((tier[0] == t).sum()) for t in range(3)]
    assert counts[0] >= 1_000_000 and counts[1] >= 1000 and counts[2] >= 1000, counts
    if batch == 2:
        single = tier[0][tiny.size:tiny.size + mixed.size].reshape(-1, 2)[:, 0]   # every mixed group left the seedless tier, for the one its element needs
        with np.errstate(invalid="ignore"):
            v = np.repeat(edge, 2)
            assert np.array_equal(single, np.where((v > 0) & (np.sqrt(np.abs(v)) < 0.5) & np.isfinite(v), 1, 2))


def test_four_tangent_group_gives_the_bits_of_tri_tan_nr_and_its_atan_tiers(forms):
    rng = np.random.default_rng(44)
    n_tiny = 1_000_000
    # cells of 1/24 to 1/3 degree: d = theta^2 / 2, the tangent about theta^2 / 4 of a half-cell triangle, so num = t den
    theta = np.deg2rad(10.0 ** rng.uniform(np.log10(1 / 24), np.log10(1 / 3), n_tiny))
    den = _b_of(theta ** 2 / 2 * rng.uniform(0.7, 1.0, n_tiny), True)
    num = theta ** 2 / 4 * rng.uniform(0.5, 1.5, n_tiny) * den
    edge_b = _edge_denominators(True)
    edge_b = edge_b[(_d_of(edge_b, True) >= 0) & (_d_of(edge_b, True) < D_TIER)]
    edge_b = edge_b[:edge_b.size // 4 * 4]
    far = _far_denominators(True)
    far = far[~((far == 0) | np.isnan(far) | np.isinf(far))]                      # the kernel's zero denominators come back as NaN tangents: below
    mixed_d = np.full((far.size * 4, 4), _b_of(1.5e-6, True))                     # exactly one far denominator at each position of a group
    for k, val in enumerate(np.repeat(far, 4)):
        mixed_d[k, k % 4] = val
    coarse = np.deg2rad(10.0 ** rng.uniform(np.log10(0.5), np.log10(80.0), 12000))  # whole groups on div_nr: coarse cells, up to the atan fallback
    coarse_d = 4.0 - 2.0 * coarse ** 2
    odd = np.array([0.0, np.nan, np.inf, -3.0] * 4)                               # a degenerate triangle, a NaN, a triangle beyond a hemisphere
    den = np.concatenate([den, edge_b, mixed_d.ravel(), coarse_d, odd])
    num = np.concatenate([num, rng.uniform(1e-9, 1e-5, edge_b.size), np.full(mixed_d.size, 1.5e-6), coarse ** 2 * rng.uniform(0.5, 1.5, coarse.size) * 4.0,
                          np.full(odd.size, 1e-6)])
    assert den.size % 4 == 0
    den, num = np.ascontiguousarray(den), np.ascontiguousarray(num)
    out, tier = np.zeros((4, den.size)), np.full((4, den.size), -1, dtype=np.int32)
    forms.tan_callers(num, den, den.size, out, tier)
    for new, old, what in ((0, 1, "tangents"), (2, 3, "atans")):
        bad = np.flatnonzero(~_same(out[new], out[old]))
        assert bad.size == 0, (what, bad.size, num[bad[:5]].tolist(), den[bad[:5]].tolist(), out[new][bad[:5]].tolist(), out[old][bad[:5]].tolist())
    d = _d_of(den, True)
    ok = ((d >= 0) & (d < D_TIER)).reshape(-1, 4).all(axis=1).repeat(4)
    assert np.array_equal(tier[0] == 0, ok) and np.array_equal(tier[0] == 1, ~ok) and (tier[1] == 1).all()
    assert np.array_equal(tier[2], tier[3])                                       # the atan tiers behind it: as they were
    assert int((tier[0] == 0).sum()) >= 1_000_000 and int((tier[0] == 1).sum()) >= 1000
    assert all(int((tier[2] == t).sum()) >= 1000 for t in (0, 1, 2)), [int((tier[2] == t).sum()) for t in range(3)]
    first = tier[0][n_tiny + edge_b.size:n_tiny + edge_b.size + mixed_d.size]
    assert (first == 1).all()                                                     # one far denominator sends its whole group to div_nr


# ---- GPU: the helpers in place, and every tier of the kernel on whole padded arrays ------------------------------------------------
F_DIV_NR, B_DIV_NEAR1, B_DIV_NEAR4 = 21, 112, 113                                # csrc/tpg_probe.hip


@pytest.mark.gpu
@pytest.mark.parametrize("quarter", [False, True], ids=["c1", "c025"])
def test_device_forms_equal_the_device_div_nr_on_the_edge_set(gpu, quarter):
    import torch
    from tools import testlib
    lib = testlib.lib()
    a, b = _edge_pairs(quarter, 7)
    far = _far_denominators(quarter)
    far = far[~((far == 0) | np.isnan(far) | np.isinf(far))]                      # div_nr's own range: finite, non-zero
    a, b = np.concatenate([a, np.ones(far.size)]), np.concatenate([b, far])
    if a.size % 2:
        a, b = a[:-1], b[:-1]
    x = np.ascontiguousarray(np.stack([a, b], axis=1).ravel())                   # pairs (a, b); a batch is two pairs
    xd = torch.from_numpy(x).to(gpu)
    res = []
    for which in (B_DIV_NEAR4 if quarter else B_DIV_NEAR1, F_DIV_NR):
        yd, rd = torch.empty_like(xd), torch.zeros(xd.numel(), dtype=torch.int32, device=gpu)
        assert lib.tpg_math_probe(which, xd.data_ptr(), yd.data_ptr(), rd.data_ptr(), xd.numel(), None) == 0
        torch.cuda.synchronize()
        res.append((yd.cpu().numpy(), rd.cpu().numpy() != 0))
    (y, rare), (want, _) = res
    d = _d_of(b, quarter)
    ok = ((d >= 0) & (d < D_TIER)).reshape(-1, 2).all(axis=1).repeat(4)           # per batch of two pairs, per slot of x
    assert np.array_equal(~rare, ok) and ok.sum() > 200_000 and (~ok).sum() > 200_000
    inside = (np.abs(d) < D_HELPER).repeat(2)                                     # the helper itself holds on all of its domain, tier test or not
    assert inside.sum() > 400_000
    bad = np.flatnonzero(inside & (_bits(y) != _bits(want)))
    assert bad.size == 0, (bad.size, x[bad[:6]].tolist(), y[bad[:6]].tolist(), want[bad[:6]].tolist())
    nz = ~((a == 0) & np.signbit(a))                                              # a = -0: +0 through both forms, see the docstring
    assert np.array_equal(_bits(want[0::2])[nz], _bits(a / b)[nz]) and np.array_equal(_bits(y[0::2]), _bits(y[1::2]))


H4 = (4, 4, 4)
# (size, float32?, (ranks, rank) of a latitude band or None, what the shape is there for)
SHAPES = [((1440, 720, 1), False, (48, 30), "tiny"),                             # rows 451 .. 465
          ((3600, 1800, 1), False, (120, 119), "tiny"),                          # rows 1786 .. 1800: row Ny, the fold, the pole-adjacent cells
          ((3600, 1800, 1), False, (120, 0), "tiny"),                            # rows 1 .. 15: the southern edge
          ((800, 400, 1), False, None, "mixed"),
          ((480, 240, 1), False, None, "most second"), ((60, 30, 1), False, None, "second"),
          ((482, 240, 1), True, None, "most second")]
CASES = [s + (order,) for s in SHAPES for order in (0, 1)]
# shares of the 30-column blocks of the interior rows that are wholly on the seedless tier, per site
PREMISE_HOLDS = {"tiny": lambda s: s == 1.0, "mixed": lambda s: 0.1 <= s <= 0.9, "most second": lambda s: 0.0 < s < 0.1, "second": lambda s: s == 0.0}


def _id(case):
    size, f32, band, _, order = case
    return f"{size[0]}x{size[1]}" + ("-f32" if f32 else "") + (f"-band{band[1]}of{band[0]}" if band else "") + f"-order{order}"


def _band_rows(case):
    size, _, band = case[:3]
    ny = size[1] // band[0]
    return band[1] * ny + 1, band[1] * ny + ny


_ref = {}


def _reference(oracle, case):
    """the oracle's arrays of a shape: computed once, shared by the two tile orders, left unchanged; the premise is asserted on the way"""
    size, f32, band, premise, _ = case
    key = _id(case)[:-len("-order0")]
    if key not in _ref:
        rows = dict(zip(("jstart", "jend"), _band_rows(case))) if band else {}
        ref = oracle.build_grid(size, dtype=np.float32 if f32 else np.float64, halo=H4, **rows)
        nrows = (rows["jend"] - rows["jstart"] + 1) if band else size[1]
        inner = lambda n: ref[n][H4[1]:H4[1] + nrows, H4[0]:H4[0] + size[0]].astype(np.float64)       # noqa: E731
        dx = np.stack([inner(n) for n in ("dx_cc", "dx_fc", "dx_cf", "dx_ff")]).max(axis=0)
        dy = np.stack([inner(n) for n in ("dy_cc", "dy_fc", "dy_cf", "dy_ff")]).max(axis=0)
        assert np.isfinite(dx).all() and np.isfinite(dy).all()
        hav = np.sin(np.maximum(dx, dy) / (2 * oracle.R_EARTH)) < R_TINY
        tri = (dx ** 2 + dy ** 2) / (4 * oracle.R_EARTH ** 2) < D_TIER
        nb = size[0] // 30
        for site, m in (("haversines", hav), ("triangles", tri)):
            share = float(m[:, :nb * 30].reshape(nrows, nb, 30).all(axis=2).mean())
            assert PREMISE_HOLDS[premise](share), (key, site, premise, share)
        for a in ref.values():
            a.setflags(write=False)
        _ref[key] = ref
    return _ref[key]


def test_cases_are_the_ones_each_tier_needs():
    assert [_band_rows(c) for c in CASES if c[2] and c[4] == 0] == [(451, 465), (1786, 1800), (1, 15)]
    assert [c[0][:2] for c in CASES if c[1]] == [(482, 240)] * 2
    assert {c[4] for c in CASES} == {0, 1} and len(CASES) == 2 * len(SHAPES) == 14
    assert {s[3] for s in SHAPES} == set(PREMISE_HOLDS)


def _arrays(osg, case):
    import torch
    size, f32, band = case[:3]
    arch = osg.GPU(0) if band is None else osg.Distributed(osg.GPU(0), osg.Partition(y=band[0]), local_rank=band[1])
    g = osg.TripolarGrid(arch, torch.float32 if f32 else torch.float64, size=size, halo=H4)
    return {n: getattr(g, n).cpu().numpy() for n in osg._lib.ARRAY_NAMES}, (g.jrange if band else None)


def _assert_same(got, want, what):
    assert len(want) == 20 and set(got) == set(want)
    for name, r in want.items():
        a = got[name]
        assert a.shape == r.shape and a.dtype == r.dtype, (what, name)
        same = _bits(a) == _bits(r)
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())


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
def test_all_twenty_arrays_equal_the_oracle_and_the_thread_per_cell_kernel(osg, oracle, gpu, knobs, case):
    want = _reference(oracle, case)
    knobs(TPG_CELLS_VARIANT=2, TPG_CELLS_ORDER=case[4])
    got, jrange = _arrays(osg, case)
    if case[2]:
        assert tuple(jrange) == _band_rows(case)
    _assert_same(got, want, "oracle")
    knobs(TPG_CELLS_VARIANT=0)
    cell, _ = _arrays(osg, case)
    _assert_same(got, cell, "thread per cell")
