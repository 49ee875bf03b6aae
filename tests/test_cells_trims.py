"""The second round of instruction trims of k_cells_tile (csrc/tpg_grid.hip, csrc/tpg_batch.hpp; profiles/cells_trims2/README.md): only
the way a result is selected, signed or scheduled changed, so every bit must be what it was.

CPU: the rewritten helpers are compiled for the host next to a copy of the forms they replace and compared bit for bit --
  * sincosd_b (one compare ladder, sin / cos swap and signs from it, signs as xor) against the two-ladder form, on every multiple of 0.25
    degrees in [-720, 720], the +-1 ulp neighbours of every multiple of 45 degrees and 10^5 seeded random angles; the POS form on |x|;
  * the longitude chain of points_pair: the sign of atan(y / x) carried by the constant and one xor instead of a rebuilt operand, and
    the first fmod360 dropped where |fplp90| < 179 keeps |l| < 360.
GPU: all 20 whole padded arrays of tpg_build_grid against the oracle and against the thread-per-cell kernel (TPG_CELLS_VARIANT=0 of the
test library), at the smallest shapes that run every trimmed path: Nx = 60 / 64 / 124 (a whole last tile, a partial one, two tiles with
a partial second) x Ny = 15..21 at halo 4 (the southernmost tile row has every residue of 1..7 active rows: the apron wave's pairs and
its single row), Float32 at Nx = 2 (mod 4), first-pole longitudes on both sides of the |fplp90| < 179 branch -- a multiple of 45 and a
non-integer on each -- and 360 x 180.  3600 x 1800 is tests/test_gpu_grid.py's."""
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
// sincosd_b as it was before the trims: two compare ladders, factors +-1.0 applied as products
template <int N> void sincosd_b(const double (&x)[N], double (&sn)[N], double (&cs)[N])
{
    double h[N], l[N], S[N], C[N], r[N], d[N];
    bool sodd[N], s_ge3[N], s_eq2[N], codd[N], c_eq1[N], c_eq2[N];
    for (int e = 0; e < N; ++e) {
        r[e] = absD(x[e]);
        const bool s1 = r[e] >= 45.0, s2 = r[e] > 135.0, s3 = r[e] >= 225.0, s4 = r[e] > 315.0;
        const bool c1 = r[e] > 45.0, c2 = r[e] >= 135.0, c3 = r[e] > 225.0, c4 = r[e] >= 315.0;
        sodd[e] = (s1 != s2) != (s3 != s4); s_ge3[e] = s3; s_eq2[e] = s2 && !s3;
        codd[e] = (c1 != c2) != (c3 != c4); c_eq1[e] = c1 && !c2; c_eq2[e] = c2 && !c3;
        double m90 = 0.0;
        m90 = s1 ? 90.0 : m90; m90 = s2 ? 180.0 : m90; m90 = s3 ? 270.0 : m90; m90 = s4 ? 360.0 : m90;
        d[e] = m90 - r[e];
        double t = absD(d[e]);
        double hh = t * kDeg2Rad;
        l[e] = fmaD(t, kDeg2Rad, -hh) + t * kDeg2RadLo;
        h[e] = hh;
    }
    tpgb::ksin_b<N>(h, l, S);
    tpgb::kcos_b<N>(h, l, C);
    for (int e = 0; e < N; ++e) {
        const double sg = csign(1.0, x[e]), nsg = -sg;
        const double dsg = csign(1.0, d[e]);
        const double bs = sodd[e] ? C[e] : S[e];
        const double f2 = dsg * sg;
        double fs = sg;
        fs = s_ge3[e] ? nsg : fs;
        fs = s_eq2[e] ? f2 : fs;
        sn[e] = fs * bs;
        const double bc = codd[e] ? S[e] : C[e];
        const double a1 = 90.0 - r[e], a3 = r[e] - 270.0;
        const double arg = c_eq1[e] ? a1 : a3;
        const double fodd = csign(1.0, arg);
        const double feven = c_eq2[e] ? -1.0 : 1.0;
        const double fc = codd[e] ? fodd : feven;
        cs[e] = fc * bc;
    }
}
// the longitude of points_pair as it was: |at1| given the sign word, then -180/pi at1 + hemi + fplp90 through both fmods
double longitude(double t, int sg, double hemi, double fplp90)
{
    const double at1 = __hiloint2double((__double2hiint(t) & 0x7fffffff) | (sg & (int)0x80000000), __double2loint(t));
    double l = -(180.0 / kPi) * at1;
    l += hemi;
    l += fplp90;
    return tpgb::fmod360_pos(tpgb::fmod360_small(l) + 360.0);
}
}  // namespace previous

// ... and as points_pair has it now: lane part and row part of the sign word apart (bit 31 only), small = |fplp90| < 179
static double longitude_now(double t, int sg_lane, int sg_row, double hemi, double fplp90)
{
    const double kC = -(180.0 / kPi);
    const double cJ = __hiloint2double(__double2hiint(kC) ^ sg_row, __double2loint(kC));
    const double m = cJ * absD(t);
    double l = __hiloint2double(__double2hiint(m) ^ sg_lane, __double2loint(m));
    l += hemi;
    l += fplp90;
    const bool lsmall = (__double2hiint(fplp90) & 0x7fffffff) < 0x40666000;
    return lsmall ? tpgb::fmod360_pos(l + 360.0) : tpgb::fmod360_pos(tpgb::fmod360_small(l) + 360.0);
}

extern "C" {
// out[0..1]: sin, cos now; [2..3]: before; [4..5]: now, POS form on |x|; [6..7]: before on |x|
void sincosd_forms(const double* x, long n, double* out)
{
    for (long i = 0; i + 1 < n; i += 2) {
        double a[2] = { x[i], x[i + 1] }, s[2], c[2];
        tpgb::sincosd_b<2>(a, s, c);
        out[0 * n + i] = s[0]; out[0 * n + i + 1] = s[1]; out[1 * n + i] = c[0]; out[1 * n + i + 1] = c[1];
        previous::sincosd_b<2>(a, s, c);
        out[2 * n + i] = s[0]; out[2 * n + i + 1] = s[1]; out[3 * n + i] = c[0]; out[3 * n + i + 1] = c[1];
        double b[2] = { absD(x[i]), absD(x[i + 1]) };
        tpgb::sincosd_b<2, true>(b, s, c);
        out[4 * n + i] = s[0]; out[4 * n + i + 1] = s[1]; out[5 * n + i] = c[0]; out[5 * n + i + 1] = c[1];
        previous::sincosd_b<2>(b, s, c);
        out[6 * n + i] = s[0]; out[6 * n + i + 1] = s[1]; out[7 * n + i] = c[0]; out[7 * n + i + 1] = c[1];
    }
}
// t: |atan| values in [0, pi/2]; bits 0 / 1 of sgn[i]: the lane's and the row's sign; out[0]: now, out[1]: before
void longitude_forms(const double* t, const int* sgn, long n, double hemi, double fplp90, double* out)
{
    for (long i = 0; i < n; ++i) {
        const int lane = (sgn[i] & 1) ? (int)0x80000000 : 0, row = (sgn[i] & 2) ? (int)0x80000000 : 0;
        out[i] = longitude_now(t[i], lane, row, hemi, fplp90);
        out[n + i] = previous::longitude(t[i], (lane ^ row) | 0x12345, hemi, fplp90);     // the old word carried other bits too
    }
}
}
"""


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """the helpers of csrc/tpg_batch.hpp compiled for the host (no contraction, as csrc/Makefile), beside their previous forms"""
    d = tmp_path_factory.mktemp("trims")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(_HIP_STUB)
    (d / "harness.cpp").write_text(_HARNESS)
    so = d / "libtrims.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wno-unknown-pragmas",
                        "-I", str(d), "-I", CSRC, "-o", str(so), str(d / "harness.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.sincosd_forms.argtypes = [dp, C.c_long, dp]
    lib.sincosd_forms.restype = None
    lib.longitude_forms.argtypes = [dp, np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS"), C.c_long, C.c_double, C.c_double, dp]
    lib.longitude_forms.restype = None
    return lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _angles():
    quarter = np.arange(-2880, 2881, dtype=np.float64) * 0.25                    # every multiple of 0.25 in [-720, 720], exact
    m45 = np.arange(-16, 17, dtype=np.float64) * 45.0
    near = np.concatenate([np.nextafter(m45, np.inf), np.nextafter(m45, -np.inf)])
    rng = np.random.default_rng(20240607)
    rnd = rng.uniform(-720.0, 720.0, 100000)
    x = np.concatenate([quarter, near, rnd, [0.0, -0.0]])
    if x.size % 2:
        x = np.append(x, 360.0)
    return np.ascontiguousarray(x)


def test_sincosd_single_ladder_equals_two_ladder_form(forms):
    x = _angles()
    out = np.zeros((8, x.size))
    forms.sincosd_forms(x, x.size, out)
    assert not np.isnan(out).any()
    for now, before, what in ((0, 2, "sind"), (1, 3, "cosd"), (4, 6, "sind, POS form"), (5, 7, "cosd, POS form")):
        bad = np.flatnonzero(_bits(out[now]) != _bits(out[before]))
        assert bad.size == 0, (what, bad.size, x[bad[:5]].tolist(), out[now][bad[:5]].tolist(), out[before][bad[:5]].tolist())
    # the exact-degree results, signed zeros included
    for deg, s, c in ((0.0, 0.0, 1.0), (90.0, 1.0, 0.0), (180.0, 0.0, -1.0), (270.0, -1.0, 0.0), (-90.0, -1.0, 0.0), (-180.0, -0.0, -1.0)):
        i = int(np.flatnonzero(x == deg)[0])                                     # the first 0.0 is the grid's +0
        assert _bits(out[0][i:i + 1])[0] == _bits(np.array([s]))[0] and _bits(out[1][i:i + 1])[0] == _bits(np.array([c]))[0], deg


@pytest.mark.parametrize("fplp90", [160.0, 45.0, -178.9, 0.0, 178.999, 179.0, 225.0, -360.0, 190.7, 360.0])
def test_longitude_chain_equals_previous_form(forms, fplp90):
    rng = np.random.default_rng(7)
    pio2 = float(np.float64.fromhex("0x1.921fb54442d18p+0"))
    t = np.concatenate([[0.0, pio2, np.nextafter(pio2, 0.0), 5e-324, 1e-17], rng.uniform(0.0, pio2, 20000)])
    for hemi in (-90.0, 90.0):
        for s in range(4):
            sgn = np.full(t.size, s, dtype=np.int32)
            out = np.zeros((2, t.size))
            forms.longitude_forms(t, sgn, t.size, hemi, fplp90, out)
            bad = np.flatnonzero(_bits(out[0]) != _bits(out[1]))
            assert bad.size == 0, (hemi, s, bad.size, t[bad[:5]].tolist())
            assert (out[0] >= 0.0).all() and not np.signbit(out[0]).any()       # what the POS form of sincosd_b relies on


# ---- GPU: every trimmed path, whole padded arrays ----------------------------------------------------------------------------------
H4 = (4, 4, 4)
# (size, extra keywords, float32?)
CASES = [((nx, ny, 1), {}, False) for nx in (60, 64, 124) for ny in range(15, 22)]
CASES += [((62, 18, 1), {}, True)]                                               # Float32, Nx = 2 (mod 4)
CASES += [((124, 20, 1), dict(first_pole_longitude=fpl), False) for fpl in (-45.0, 70.3, 135.0, 100.7)]   # fplp90 = 45, 160.3 | 225, 190.7
CASES += [((360, 180, 1), {}, False)]


def _id(case):
    size, kw, f32 = case
    return f"{size[0]}x{size[1]}" + ("-f32" if f32 else "") + (f"-fpl{kw['first_pole_longitude']}" if kw else "")


_ref = {}


def _reference(oracle, case):
    """the oracle's arrays of a case: computed once, shared by both tests, left unchanged"""
    size, kw, f32 = case
    if _id(case) not in _ref:
        ref = oracle.build_grid(size, dtype=np.float32 if f32 else np.float64, halo=H4, **kw)
        for a in ref.values():
            a.setflags(write=False)
        _ref[_id(case)] = ref
    return _ref[_id(case)]


def _arrays(osg, case):
    import torch
    size, kw, f32 = case
    g = osg.TripolarGrid(osg.GPU(0), torch.float32 if f32 else torch.float64, size=size, halo=H4, **kw)
    return {n: getattr(g, n).cpu().numpy() for n in osg._lib.ARRAY_NAMES}


def _assert_same(got, want, what):
    assert len(want) == 20 and set(got) == set(want)
    for name, r in want.items():
        a = got[name]
        assert a.shape == r.shape and a.dtype == r.dtype, (what, name)
        same = _bits(a) == _bits(r)
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_twenty_arrays_equal_the_oracle_bit_for_bit(osg, oracle, gpu, case):
    _assert_same(_arrays(osg, case), _reference(oracle, case), "oracle")


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
    want = _arrays(osg, case)
    cells_variant(2)
    _assert_same(_arrays(osg, case), want, "thread per cell")
