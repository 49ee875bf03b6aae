"""The third round of instruction trims of k_cells_tile (csrc/tpg_grid.hip, csrc/tpg_batch.hpp; profiles/cells_trims3/README.md): only
the way a result is selected, signed, addressed or checked for a rare argument changed, so every bit must be what it was.

CPU: every changed helper is compiled for the host next to a copy of the form it replaces and compared bit for bit --
  * sincosd_lat_b: the sine's sign as a copysign instead of a product with +-1.0;
  * atan_small_b<N, true>: +0 <= x < 0.4375 as one unsigned compare of the high word, no |x| and no copysign; with the caller's fallback
    (atan_b) around both forms, since the new form sends negative arguments there;
  * atan_tab_b<N, FINITE, true>: |atan(x)| without the copysign, against |.| of the signed form;
  * asin_sqrt_b, the tail of a haversine: ONE test r < 0.5 on the unscaled square root instead of h == 0, min(r, 1) and |r| < 0.5;
    every argument that took the zero patch or the scalar asin before must fail the new test.
Arguments, each helper: every multiple of 0.25 in [-720, 720], the +-1 ulp neighbours of every multiple of 45, 10^5 seeded random
values, the same sets scaled into the helper's own domain, and both sides of every threshold of a merged or rewritten check.
GPU: all 20 whole padded arrays of tpg_build_grid against the oracle and against the thread-per-cell kernel (TPG_CELLS_VARIANT=0 of the
test library) at Nx = 60 / 64 / 124 x Ny = 15..21, Float32 at Nx = 62, four first-pole longitudes (fplp90 = 45, 160.3, 190.7, 225),
360 x 180, and latitude bands with jstart = 1 (the south apron row of the lowest tile row is row 0, the zero south halo, which the tile
kernel now takes on its paired path with constants for the two Center-y points) and with jstart > Hy + 1 (an ordinary apron row).
3600 x 1800 is tests/test_gpu_grid.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")

# ---- CPU: new helper forms against the forms they replace ---------------------------------------------------------------------------
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
using namespace tpgm;

namespace previous {
// sincosd_lat_b as it was: the sine's sign as a product with +-1.0
template <int N> bool sincosd_lat_b(const double (&x)[N], double (&sn)[N], double (&cs)[N])
{
    double h[N], l[N], S[N], C[N];
    bool s1[N], c1[N], rare = false;
    for (int e = 0; e < N; ++e) {
        const double r = absD(x[e]);
        rare |= !(r <= 90.0);
        s1[e] = r >= 45.0; c1[e] = r > 45.0;
        const double d = (s1[e] ? 90.0 : 0.0) - r;
        const double t = absD(d);
        const double hh = t * kDeg2Rad;
        l[e] = fmaD(t, kDeg2Rad, -hh) + t * kDeg2RadLo;
        h[e] = hh;
    }
    tpgb::ksin_b<N>(h, l, S);
    tpgb::kcos_b<N>(h, l, C);
    for (int e = 0; e < N; ++e) {
        const double bs = s1[e] ? C[e] : S[e];
        sn[e] = csign(1.0, x[e]) * bs;
        cs[e] = c1[e] ? S[e] : C[e];
    }
    return rare;
}
// atan_small_b as it was: |x| < 0.4375, t = |x|, the result given the sign of x
template <int N> bool atan_small_b(const double (&x)[N], double (&out)[N])
{
    double t[N], z[N], w[N], s1[N], s2[N];
    bool rare = false;
    for (int e = 0; e < N; ++e) { t[e] = absD(x[e]); rare |= !(t[e] < 0.4375); }
    for (int e = 0; e < N; ++e) { z[e] = t[e] * t[e]; w[e] = z[e] * z[e]; }
    for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], 1.62858201153657823623e-02, 4.97687799461593236017e-02);
                                  s2[e] = fmaD(w[e], -3.65315727442169155270e-02, -5.83357013379057348645e-02); }
    for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 6.66107313738753120669e-02); s2[e] = fmaD(w[e], s2[e], -7.69187620504482999495e-02); }
    for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 9.09088713343650656196e-02); s2[e] = fmaD(w[e], s2[e], -1.11111104054623557880e-01); }
    for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 1.42857142725034663711e-01); s2[e] = fmaD(w[e], s2[e], -1.99999999998764832476e-01); }
    for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 3.33333333333329318027e-01); s2[e] = w[e] * s2[e]; }
    for (int e = 0; e < N; ++e) {
        const double sm = z[e] * s1[e] + s2[e];
        const double r = t[e] - t[e] * sm;
        out[e] = csign(r, x[e]);
    }
    return rare;
}
// the tail of hav_batch as it was: the zero patch of the unscaled square root, min(r, 1) as minnum, asin_small_b's own |x| < 0.5 and the
// scalar fallback; flags: bit 0 the zero patch ran, bit 1 the scalar asin ran
template <int N> int asin_sqrt(const double (&hh)[N], double (&as)[N])
{
    double rt[N], rm[N];
    bool zero = false;
    for (int e = 0; e < N; ++e) { zero |= hh[e] == 0.0; rt[e] = sqrt_nr<true>(hh[e]); }
    if (zero) for (int e = 0; e < N; ++e) rt[e] = sqrt_nr(hh[e]);
    for (int e = 0; e < N; ++e) rm[e] = __builtin_fmin(rt[e], 1.0);
    const bool rare = tpgb::asin_small_b<N>(rm, as);
    if (rare) for (int e = 0; e < N; ++e) as[e] = asinD(!(rt[e] >= 1.0) ? rt[e] : 1.0);
    return (zero ? 1 : 0) | (rare ? 2 : 0);
}
}  // namespace previous

extern "C" {
// out[0..1]: sin, cos now; [2..3]: before; rare[0]: now, rare[1]: before.  One-element batches, the kernel's form
void sincosd_lat_forms(const double* x, long n, double* out, int* rare)
{
    for (long i = 0; i < n; ++i) {
        double a[1] = { x[i] }, s[1], c[1];
        rare[i] = tpgb::sincosd_lat_b<1>(a, s, c); out[i] = s[0]; out[n + i] = c[0];
        rare[n + i] = previous::sincosd_lat_b<1>(a, s, c); out[2 * n + i] = s[0]; out[3 * n + i] = c[0];
    }
}
// out[0]: atan_small_b<4, true> with the caller's fallback; [1]: the previous form with it; [2], [3]: the two without it.  Batches of 4.
void atan_small_forms(const double* x, long n, double* out, int* rare)
{
    for (long i = 0; i + 3 < n; i += 4) {
        double a[4] = { x[i], x[i + 1], x[i + 2], x[i + 3] }, o[4], f[4];
        tpgb::atan_b<4>(a, f);
        const bool rn = tpgb::atan_small_b<4, true>(a, o);
        for (int e = 0; e < 4; ++e) { out[i + e] = rn ? f[e] : o[e]; out[2 * n + i + e] = o[e]; rare[i + e] = rn; }
        const bool rp = previous::atan_small_b<4>(a, o);
        for (int e = 0; e < 4; ++e) { out[n + i + e] = rp ? f[e] : o[e]; out[3 * n + i + e] = o[e]; rare[n + i + e] = rp; }
    }
}
// out[0]: the ABS form; [1]: the signed form (the code of before: the flag only skips its last operation); [2], [3]: the FINITE forms
void atan_tab_forms(const double* x, long n, double* out)
{
    double tab[TPG_ATAN_TABLE_DOUBLES];
    for (int t = 0; t < 64; ++t) tpgb::atan_table_init(tab, t);
    for (long i = 0; i + 1 < n; i += 2) {
        double a[2] = { x[i], x[i + 1] }, o[2];
        tpgb::atan_tab_b<2, false, true>(a, o, tab);  out[i] = o[0]; out[i + 1] = o[1];
        tpgb::atan_tab_b<2, false, false>(a, o, tab); out[n + i] = o[0]; out[n + i + 1] = o[1];
        tpgb::atan_tab_b<2, true, true>(a, o, tab);   out[2 * n + i] = o[0]; out[2 * n + i + 1] = o[1];
        tpgb::atan_tab_b<2, true, false>(a, o, tab);  out[3 * n + i] = o[0]; out[3 * n + i + 1] = o[1];
    }
}
// out[0]: asin_sqrt_b now; [1]: before; flags[0]: the fallback ran now; flags[1]: bits of previous::asin_sqrt.  Batches of 2.
void asin_sqrt_forms(const double* h, long n, double* out, int* flags)
{
    for (long i = 0; i + 1 < n; i += 2) {
        double a[2] = { h[i], h[i + 1] }, o[2];
        const bool rn = tpgb::asin_sqrt_b<2>(a, o);
        out[i] = o[0]; out[i + 1] = o[1]; flags[i] = flags[i + 1] = rn;
        const int fp = previous::asin_sqrt<2>(a, o);
        out[n + i] = o[0]; out[n + i + 1] = o[1]; flags[n + i] = flags[n + i + 1] = fp;
    }
}
}
"""


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """the helpers of csrc/tpg_batch.hpp compiled for the host (no contraction, as csrc/Makefile), beside their previous forms"""
    d = tmp_path_factory.mktemp("trims3")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(_HIP_STUB)
    (d / "harness.cpp").write_text(_HARNESS)
    so = d / "libtrims3.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wno-unknown-pragmas",
                        "-Wno-attributes", "-I", str(d), "-I", CSRC, "-o", str(so), str(d / "harness.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    for name, args in (("sincosd_lat_forms", [dp, C.c_long, dp, ip]), ("atan_small_forms", [dp, C.c_long, dp, ip]),
                       ("atan_tab_forms", [dp, C.c_long, dp]), ("asin_sqrt_forms", [dp, C.c_long, dp, ip])):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = None
    return lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    """bit for bit; two NaNs count as the same result"""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _angles():
    """the issue's argument sets: every multiple of 0.25 in [-720, 720] (exact), the +-1 ulp neighbours of the multiples of 45, 10^5 random"""
    quarter = np.arange(-2880, 2881, dtype=np.float64) * 0.25
    m45 = np.arange(-16, 17, dtype=np.float64) * 45.0
    near = np.concatenate([np.nextafter(m45, np.inf), np.nextafter(m45, -np.inf)])
    rnd = np.random.default_rng(20250311).uniform(-720.0, 720.0, 100000)
    return np.concatenate([quarter, near, rnd, [0.0, -0.0]])


def _around(*thresholds):
    t = np.array(thresholds, dtype=np.float64)
    return np.concatenate([t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf), -t, -np.nextafter(t, np.inf), -np.nextafter(t, -np.inf)])


def _pad(x, k):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([x, np.full((-x.size) % k, x[-1])]))


def test_sincosd_lat_copysign_equals_the_product_form(forms):
    # latitudes proper (the kernel's domain, |x| <= 90: the angle sets scaled by 1/8) and the sets themselves (|x| > 90: rare in both)
    a = _angles()
    x = _pad(np.concatenate([a / 8.0, a, _around(45.0, 90.0), [5e-324, -5e-324, 1e-310, np.nan, np.inf, -np.inf]]), 1)
    out, rare = np.zeros((4, x.size)), np.zeros((2, x.size), dtype=np.int32)
    forms.sincosd_lat_forms(x, x.size, out, rare)
    assert np.array_equal(rare[0], rare[1]) and np.array_equal(rare[0] != 0, ~(np.abs(x) <= 90.0))
    fast = rare[0] == 0
    assert fast.sum() > 100000
    for now, before, what in ((0, 2, "sind"), (1, 3, "cosd")):
        bad = np.flatnonzero(fast & (_bits(out[now]) != _bits(out[before])))
        assert bad.size == 0, (what, bad.size, x[bad[:5]].tolist())
    assert np.signbit(out[0][fast]).tolist() == np.signbit(x[fast]).tolist()      # -0 -> -0, +0 -> +0 included


def test_atan_small_positive_form_equals_previous_form(forms):
    a = _angles()
    # the tangents of the kernel are O(1e-6) and positive; the sets scaled by 1e-3 straddle 0.4375 with both signs
    x = _pad(np.concatenate([a * 1e-3, a * 1e-8, a, _around(0.4375, 0.0, 5e-324, 2.0 ** -27, 1.0), [np.nan, np.inf, -np.inf]]), 4)
    out, rare = np.zeros((4, x.size)), np.zeros((2, x.size), dtype=np.int32)
    forms.atan_small_forms(x, x.size, out, rare)
    bad = np.flatnonzero(~_same(out[0], out[1]))                                 # with the fallback around both: the same bits everywhere
    assert bad.size == 0, (bad.size, x[bad[:5]].tolist(), out[0][bad[:5]].tolist(), out[1][bad[:5]].tolist())
    assert not (rare[1] & ~rare[0] & 1).any()                                    # what took the fallback before still takes it
    grp = ((x >= 0) & ~np.signbit(x) & (x < 0.4375)).reshape(-1, 4).all(axis=1).repeat(4)
    assert np.array_equal(rare[0] != 0, ~grp)                                    # and the new test is exactly +0 <= x < 0.4375
    ok = (x >= 0) & ~np.signbit(x) & (x < 0.4375)
    assert (_bits(out[2][ok]) == _bits(out[3][ok])).all()                        # the two evaluations alone, on the new fast domain
    assert (rare[0] == 0).sum() > 1000 and ((rare[0] != 0) & (rare[1] == 0)).sum() > 1000


def test_atan_tab_abs_form_is_the_magnitude_of_the_signed_form(forms):
    a = _angles()
    rng = np.random.default_rng(5)
    wide = 10.0 ** rng.uniform(-40, 80, 20000) * rng.choice([-1.0, 1.0], 20000)
    x = _pad(np.concatenate([a, a / 256.0, wide, _around(0.4375, 0.6875, 1.1875, 2.4375, 0.0, 2.0 ** 1000), [np.inf, -np.inf]]), 2)
    out = np.zeros((4, x.size))
    forms.atan_tab_forms(x, x.size, out)
    assert not np.isnan(out[:2]).any() and not np.signbit(out[0]).any()
    assert np.array_equal(_bits(out[0]), _bits(np.abs(out[1])))
    assert np.array_equal(np.signbit(out[1]), np.signbit(x))
    fin = np.abs(x) < 2.0 ** 999                                                 # FINITE: the caller's promise
    assert np.array_equal(_bits(out[2][fin]), _bits(np.abs(out[3][fin]))) and np.array_equal(_bits(out[2][fin]), _bits(out[0][fin]))


def test_haversine_tail_one_test_equals_three(forms):
    a = _angles()
    rng = np.random.default_rng(9)
    # h = sin^2 + cos cos sin^2 lies in [0, 1] (+ rounding); the fast domain is 0 < h < 0.25
    h = np.concatenate([np.abs(a) / 720.0, np.abs(a) / 2880.0, (a / 720.0) ** 2, a / 720.0, 10.0 ** rng.uniform(-34, 0.1, 20000),
                        _around(0.25, 1.0, 0.0, 1e-34, 2.0), [np.nan, np.inf, 0.0, 0.0, 0.3, 0.0, 0.0, 0.1]])
    h = _pad(h, 2)
    out, flags = np.zeros((2, h.size)), np.zeros((2, h.size), dtype=np.int32)
    forms.asin_sqrt_forms(h, h.size, out, flags)
    bad = np.flatnonzero(~_same(out[0], out[1]))
    assert bad.size == 0, (bad.size, h[bad[:5]].tolist(), out[0][bad[:5]].tolist(), out[1][bad[:5]].tolist())
    assert not ((flags[1] != 0) & (flags[0] == 0)).any()                         # zero patch or scalar asin before => fallback now
    with np.errstate(invalid="ignore"):
        grp = ((h > 0) & (np.sqrt(h) < 0.5)).reshape(-1, 2).all(axis=1).repeat(2)
    assert np.array_equal(flags[0] != 0, ~grp)                                   # the one test is exactly 0 < h and sqrt(h) < 0.5
    assert (flags[0] == 0).sum() > 10000 and (flags[1] == 1).sum() > 0 and (flags[1] >= 2).sum() > 1000


# ---- GPU: every trimmed path, whole padded arrays ----------------------------------------------------------------------------------
H4 = (4, 4, 4)
# (size, extra keywords, float32?, (ranks, rank) of a latitude band or None)
CASES = [((nx, ny, 1), {}, False, None) for nx in (60, 64, 124) for ny in range(15, 22)]
CASES += [((62, 18, 1), {}, True, None)]                                         # Float32, Nx = 2 (mod 4)
CASES += [((124, 20, 1), dict(first_pole_longitude=fpl), False, None) for fpl in (-45.0, 70.3, 135.0, 100.7)]   # fplp90 = 45, 160.3 | 225, 190.7
CASES += [((360, 180, 1), {}, False, None)]
# bands of 7 rows of a 124 x 21 grid: rank 0 has jstart = 1 (apron row 0), ranks 1 and 2 jstart = 8, 15 > Hy + 1 (an ordinary apron row);
# and of 60 x 40 in two: jstart = 21, two tile rows above an ordinary apron row
CASES += [((124, 21, 1), {}, False, (3, r)) for r in range(3)] + [((60, 40, 1), {}, False, (2, r)) for r in range(2)]
CASES += [((62, 21, 1), {}, True, (3, 0)), ((62, 21, 1), {}, True, (3, 1))]


def _id(case):
    size, kw, f32, band = case
    return (f"{size[0]}x{size[1]}" + ("-f32" if f32 else "") + (f"-fpl{kw['first_pole_longitude']}" if kw else "")
            + (f"-band{band[1]}of{band[0]}" if band else ""))


_ref = {}


def _grid(osg, case):
    import torch
    size, kw, f32, band = case
    arch = osg.GPU(0) if band is None else osg.Distributed(osg.GPU(0), osg.Partition(y=band[0]), local_rank=band[1])
    return osg.TripolarGrid(arch, torch.float32 if f32 else torch.float64, size=size, halo=H4, **kw)


def _arrays(osg, case):
    g = _grid(osg, case)
    return {n: getattr(g, n).cpu().numpy() for n in osg._lib.ARRAY_NAMES}, (g.jrange if case[3] else None)


def _reference(oracle, case, jrange):
    """the oracle's arrays of a case: computed once, shared, left unchanged"""
    size, kw, f32, band = case
    if _id(case) not in _ref:
        rows = {} if jrange is None else dict(jstart=jrange[0], jend=jrange[1])
        ref = oracle.build_grid(size, dtype=np.float32 if f32 else np.float64, halo=H4, **kw, **rows)
        for a in ref.values():
            a.setflags(write=False)
        _ref[_id(case)] = ref
    return _ref[_id(case)]


def _assert_same(got, want, what):
    assert len(want) == 20 and set(got) == set(want)
    for name, r in want.items():
        a = got[name]
        assert a.shape == r.shape and a.dtype == r.dtype, (what, name)
        same = _bits(a) == _bits(r)
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def test_band_cases_cover_both_forms_of_the_south_apron_row():
    """jstart = 1: jm_lo = 1, the lowest tile row's apron row is row 0; jstart > Hy + 1: jm_lo = jstart - Hy > 1, an ordinary row"""
    starts = set()
    for size, _, _, band in CASES:
        if band:
            ny = size[1] // band[0]
            starts.add(band[1] * ny + 1)
    assert 1 in starts and any(j > H4[1] + 1 for j in starts)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_twenty_arrays_equal_the_oracle_bit_for_bit(osg, oracle, gpu, case):
    got, jrange = _arrays(osg, case)
    if case[3]:
        ny = case[0][1] // case[3][0]
        assert tuple(jrange) == (case[3][1] * ny + 1, case[3][1] * ny + ny)
    _assert_same(got, _reference(oracle, case, jrange), "oracle")


@pytest.fixture
def cells_variant(osg, via_testlib):
    saved = os.environ.get("TPG_CELLS_VARIANT")

    def select(v):
        os.environ["TPG_CELLS_VARIANT"] = str(v)
        via_testlib.tpg_reload_config()
    yield select
    if saved is None:
        os.environ.pop("TPG_CELLS_VARIANT", None)
    else:
        os.environ["TPG_CELLS_VARIANT"] = saved
    via_testlib.tpg_reload_config()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tile_kernel_equals_the_thread_per_cell_kernel(osg, gpu, cells_variant, case):
    cells_variant(0)
    want, _ = _arrays(osg, case)
    cells_variant(2)
    got, _ = _arrays(osg, case)
    _assert_same(got, want, "thread per cell")
