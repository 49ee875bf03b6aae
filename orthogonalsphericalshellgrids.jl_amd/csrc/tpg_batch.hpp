// tpg_batch.hpp -- straight-line ("batched") forms of the tpg_math.hpp functions.
//
// The metric kernel is FP64 latency-bound: at 2 waves/SIMD a chain of dependent v_fma_f64 leaves
// the SIMD idle ~1/3 of the time, and the early-outs / range branches of the scalar functions cut
// the code into small basic blocks the scheduler cannot interleave.  Each function here evaluates
// N independent arguments in one basic block, stage by stage ("vertical" order), with selects
// instead of branches.  Every output has EXACTLY the bits of the scalar function:
//   * the msun early-outs (|x| < 2^-27, |x| >= 2^66, ...) are shortcuts, not different values: the
//     general formula rounds to the same result there (argued next to each function);
//   * where a scalar function genuinely takes another path (|x| > pi/4 in sin, |x| >= 0.5 in asin,
//     deep cancellation in the pi/2 reduction) the batch form reports a `rare` flag and the caller
//     re-evaluates through the scalar function.
#pragma once
#include "tpg_math.hpp"

namespace tpgb {
using namespace tpgm;

#define TPG_UNROLL _Pragma("unroll")

// Instrument of tools/cells_ledger.py (scratch builds only: make GRID_FLAGS=-DTPG_CELLS_NO_FALLBACK=1, in the style of TPG_CELLS_PROBE):
// no batch function reports a rare argument, so the compiler deletes every scalar fallback and what is left of a kernel is its main
// path alone, readable instruction by instruction.  Results are WRONG by design; never built into a library that a test or the bench loads.
#ifndef TPG_CELLS_NO_FALLBACK
#define TPG_CELLS_NO_FALLBACK 0
#endif
#if TPG_CELLS_NO_FALLBACK
#define TPG_RARE(r) false
#else
#define TPG_RARE(r) (r)
#endif

// A Float64 literal of a one-element batch, pinned to a scalar register pair.  A literal with a non-zero low word needs a register; used
// once, the compiler builds it in a VECTOR pair (two v_mov_b32) so that the fma can take its two-address form -- two VALU instructions per
// coefficient.  From a scalar pair the three-address fma reads it as its one scalar operand.  Batches of two and more use every
// coefficient more than once and get the scalar pair by themselves.
template <int N> TPG_DEV double kc(double c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (N == 1) asm("" : "+s"(c));
#endif
    return c;
}

// ksin / kcos of x + y, elementwise (any N)
template <int N> TPG_DEV void ksin_b(const double (&x)[N], const double (&y)[N], double (&out)[N])
{
    double z[N], r[N], v[N];
    TPG_UNROLL for (int e = 0; e < N; ++e) z[e] = x[e] * x[e];
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], kc<N>(1.58969099521155010221e-10), kc<N>(-2.50507602534068634195e-08));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(2.75573137070700676789e-06));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(-1.98412698298579493134e-04));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(8.33333333332248946124e-03));
    TPG_UNROLL for (int e = 0; e < N; ++e) v[e] = z[e] * x[e];
    TPG_UNROLL for (int e = 0; e < N; ++e)
        out[e] = x[e] - ((z[e] * (0.5 * y[e] - v[e] * r[e]) - y[e]) - v[e] * kc<N>(-1.66666666666666324348e-01));
}
template <int N> TPG_DEV void kcos_b(const double (&x)[N], const double (&y)[N], double (&out)[N])
{
    double z[N], r[N];
    TPG_UNROLL for (int e = 0; e < N; ++e) z[e] = x[e] * x[e];
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], kc<N>(-1.13596475577881948265e-11), kc<N>(2.08757232129817482790e-09));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(-2.75573143513906633035e-07));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(2.48015872894767294178e-05));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(-1.38888888888741095749e-03));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(4.16666666666666019037e-02));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = z[e] * r[e];
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        double hz = 0.5 * z[e];
        double w = 1.0 - hz;
        out[e] = w + (((1.0 - w) - hz) + (z[e] * r[e] - x[e] * y[e]));
    }
}

// sin(x) for |x| <= pi/4 (the haversine's half-differences).  tpgm::sinD returns x for
// |x| < 2^-26: ksin(x, 0) = x - x^3/6 (1 - ...) rounds to x there (|x^2/6| < 2^-54), also for +-0.
// rare: some |x| > pi/4 (seam-crossing longitude differences) -> caller uses tpgm::sinD.
// ksin(x, 0): the y = 0 form of ksin_b with the two operations on y removed.  ksin_b evaluates x - ((z (0.5 y - v r) - y) - v S1);
// with y = +0 the inner difference is 0 - v r and "- y" is the identity.  0 - t equals -t except for t = +0 (0 - 0 = +0, -(+0) = -0),
// and that sign never reaches the result: t = v r = +0 only when v = +0 (r > 0), z (-+0) is a zero of either sign, the next term
// v S1 is then -0 (S1 < 0) and (+-0) - (-0) = +0 in both cases.  So z * -(v r) gives the bits of z * (0 - v r) - 0 everywhere
// (checked argument by argument against the scalar sinD, signed zeros and subnormals included: tests/test_gpu_math.py) -- one VALU
// instruction less per sine, 16 per cell of the metric kernel.
template <int N> TPG_DEV void ksin0_b(const double (&x)[N], double (&out)[N])
{
    double z[N], r[N], v[N];
    TPG_UNROLL for (int e = 0; e < N; ++e) z[e] = x[e] * x[e];
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], kc<N>(1.58969099521155010221e-10), kc<N>(-2.50507602534068634195e-08));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(2.75573137070700676789e-06));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(-1.98412698298579493134e-04));
    TPG_UNROLL for (int e = 0; e < N; ++e) r[e] = fmaD(z[e], r[e], kc<N>(8.33333333332248946124e-03));
    TPG_UNROLL for (int e = 0; e < N; ++e) v[e] = z[e] * x[e];
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double t = v[e] * r[e];
        out[e] = x[e] - (z[e] * -t - v[e] * kc<N>(-1.66666666666666324348e-01));
    }
}

template <int N> TPG_DEV bool sin_small_b(const double (&x)[N], double (&out)[N])
{
    bool rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) rare |= !(absD(x[e]) <= kPio4Hi);
    ksin0_b<N>(x, out);
    return TPG_RARE(rare);
}

// cos(a) through the first Cody-Waite step for every argument (n = 0 reproduces the direct
// kcos(a, 0) of tpgm::cosD exactly: fn = +-0, y0 = a, y1 = 0).
// rare: the reduction would need its 2nd iteration (a within 2^-16 relative of an odd multiple of
// pi/2, e.g. the geographic pole phi = 90) -> caller uses tpgm::cosD.
template <int N> TPG_DEV bool cos_b(const double (&a)[N], double (&out)[N])
{
    double fn[N], y0[N], y1[N], S[N], C[N];
    bool rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) fn[e] = __builtin_rint(a[e] * kInvPio2);
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        double r = a[e] - fn[e] * kPio2_1;
        double w = fn[e] * kPio2_1t;
        y0[e] = r - w;
        y1[e] = (r - y0[e]) - w;
        // the scalar code iterates when the exponents of a and y0 differ by more than 16, i.e. |y0| < 2^-16 |a| (both normal);
        // |y0| < 2^-15 |a| is a superset of that (it sends a few more lanes to the scalar function, whose result the fast path
        // equals wherever it is valid) and costs a multiply and a compare instead of two exponent extractions, a subtract and a compare
        rare |= absD(y0[e]) < absD(a[e]) * 0x1p-15;
    }
    // lanes of a wave sit on neighbouring latitudes: usually every argument needs the same kernel
    bool odd = false, even = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) { const int n = (int)fn[e]; odd |= (n & 1) != 0; even |= (n & 1) == 0; }
    TPG_UNROLL for (int e = 0; e < N; ++e) { S[e] = 0.0; C[e] = 0.0; }
    if (__any(odd)) ksin_b<N>(y0, y1, S);
    if (__any(even)) kcos_b<N>(y0, y1, C);
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const int n = (int)fn[e];
        const double v = (n & 1) ? S[e] : C[e];
        const double nv = -v;
        out[e] = ((n + 1) & 2) ? nv : v;
    }
    return TPG_RARE(rare);
}

// cos(a) for a = deg2rad(latitude), |a| <= pi/2 (+ rounding): the Cody-Waite quotient n = rint(a 2/pi) is -1, 0 or +1, so the
// quadrant logic of cos_b -- convert to int, test bit 0, test bit 1 of n + 1 -- collapses to two compares of the quotient itself:
// n = 0 -> kcos(y), n = +1 -> -ksin(y), n = -1 -> +ksin(y).  Same reduction, same kernels, same bits as cos_b / tpgm::cosD.
// rare: |n| > 1 (not a latitude), or the reduction would need its 2nd iteration (see cos_b) -> caller uses tpgm::cosD.
template <int N> TPG_DEV bool cos_lat_b(const double (&a)[N], double (&out)[N])
{
    double fn[N], y0[N], y1[N], S[N], C[N];
    bool rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) fn[e] = __builtin_rint(a[e] * kInvPio2);
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        double r = a[e] - fn[e] * kPio2_1;
        double w = fn[e] * kPio2_1t;
        y0[e] = r - w;
        y1[e] = (r - y0[e]) - w;
        rare |= absD(y0[e]) < absD(a[e]) * 0x1p-15;
        rare |= !(absD(fn[e]) <= 1.0);
    }
    bool odd = false, even = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) { odd |= fn[e] != 0.0; even |= fn[e] == 0.0; }
    TPG_UNROLL for (int e = 0; e < N; ++e) { S[e] = 0.0; C[e] = 0.0; }
    if (__any(odd)) ksin_b<N>(y0, y1, S);
    if (__any(even)) kcos_b<N>(y0, y1, C);
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double v = (fn[e] != 0.0) ? S[e] : C[e];
        const double nv = -v;
        out[e] = (fn[e] > 0.0) ? nv : v;
    }
    return TPG_RARE(rare);
}

// atan(x), all x (finite, +-Inf; NaN -> NaN).  The scalar early-outs are redundant value-wise:
//  |x| < 2^-27: t - t (s1+s2) with s1+s2 ~ t^2/3 < 2^-55 rounds to t;
//  |x| >= 2^66 (and Inf): t = -1/|x| is below half an ulp of pi/2, the formula gives RN(hi + lo) = hi.
template <int N> TPG_DEV void atan_b(const double (&x)[N], double (&out)[N])
{
    double t[N], hi[N], lo[N], s[N];
    bool direct[N];
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        double ax = absD(x[e]);
        direct[e] = ax < 0.4375;
        const bool b0 = ax < 0.6875, b1 = ax < 1.1875, b2 = ax < 2.4375;
        // every candidate is computed, then chosen with plain selects (arms are variables, so the
        // compiler emits v_cndmask instead of divergent branches)
        const double n0 = 2.0 * ax - 1.0, n1 = ax - 1.0, n2 = ax - 1.5;
        const double d0 = 2.0 + ax, d1 = ax + 1.0, d2 = 1.0 + 1.5 * ax;
        double num = -1.0, den = ax, h = kPio2Hi, l = kPio2Lo;
        const double h2 = 0x1.f730bd281f69bp-1, l2 = 0x1.007887af0cbbdp-56;
        const double h1 = 0x1.921fb54442d18p-1, l1 = 0x1.1a62633145c07p-55;
        const double h0 = 0x1.dac670561bb4fp-2, l0 = 0x1.a2b7f222f65e2p-56;
        num = b2 ? n2 : num; den = b2 ? d2 : den; h = b2 ? h2 : h; l = b2 ? l2 : l;
        num = b1 ? n1 : num; den = b1 ? d1 : den; h = b1 ? h1 : h; l = b1 ? l1 : l;
        num = b0 ? n0 : num; den = b0 ? d0 : den; h = b0 ? h0 : h; l = b0 ? l0 : l;
        hi[e] = h; lo[e] = l;
        double q = num / den;
        asm volatile("" : "+v"(q));          // keep the division unconditional: no branch around it
        t[e] = direct[e] ? ax : q;
    }
    {
        double z[N], w[N], s1[N], s2[N];
        TPG_UNROLL for (int e = 0; e < N; ++e) { z[e] = t[e] * t[e]; w[e] = z[e] * z[e]; }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], 1.62858201153657823623e-02, 4.97687799461593236017e-02);
                                                 s2[e] = fmaD(w[e], -3.65315727442169155270e-02, -5.83357013379057348645e-02); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 6.66107313738753120669e-02);
                                                 s2[e] = fmaD(w[e], s2[e], -7.69187620504482999495e-02); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 9.09088713343650656196e-02);
                                                 s2[e] = fmaD(w[e], s2[e], -1.11111104054623557880e-01); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 1.42857142725034663711e-01);
                                                 s2[e] = fmaD(w[e], s2[e], -1.99999999998764832476e-01); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 3.33333333333329318027e-01);
                                                 s2[e] = w[e] * s2[e]; }
        TPG_UNROLL for (int e = 0; e < N; ++e) s[e] = z[e] * s1[e] + s2[e];
    }
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double ts = t[e] * s[e];
        const double rd = t[e] - ts, rg = hi[e] - ((ts - lo[e]) - t[e]);
        const double r = direct[e] ? rd : rg;
        out[e] = csign(r, x[e]);
    }
}

// Range-reduction constants of atan, one row per msun interval (the "direct" interval |x| < 0.4375 first):
//   t = (p*ax - q) / (r + s*ax),  result = hi - ((t*poly - lo) - t)
// (p*ax, s*ax are exact for p,s in {0,1,2}; 1.5*ax rounds exactly as the scalar code's 1.5*ax).  The direct
// interval is the row p = 1, q = 0, r = 1, s = 0, hi = lo = 0: t = ax / 1 = ax exactly and
// 0 - ((t*poly - 0) - t) is the scalar branch's t - t*poly bit for bit (both differences are exact
// negations of each other; a zero difference is +0 either way).
// Looked up per lane from LDS (3 ds_read_b128) instead of selects over the unused candidates.
struct AtanRow { double p, q, r, s, hi, lo; };
// The interval is looked up too (round 3): the four thresholds 0.4375, 0.6875, 1.1875, 2.4375 have zero low words and high words
// that are multiples of 2^15, so |x| >= T  <=>  (high word of |x|) >> 15 >= (high word of T) >> 15, and the 81 values
// u = clamp(((hi >> 15) & 0xFFFF) - 0x7FB7, 0, 80) cover all five intervals (u = 0: below 0.4375 ... u = 80: from 2.4375 up, +Inf
// and NaN included -- a NaN argument gives NaN through any row).  lut[u] = byte offset of the row: 3 integer instructions and one
// ds_read_u8 instead of 4 compares + 4 selects.  The LUT sits behind the 30 row doubles (12 more doubles per copy).
#define TPG_ATAN_ROWS_DOUBLES 30
#define TPG_ATAN_TABLE_DOUBLES 42
// The table as it lies in LDS, one constant image of TPG_ATAN_TABLE_DOUBLES 8-byte words: thread k copies word k, rows and LUT alike, so
// the copy is ONE load and ONE store per thread with no row / column arithmetic and no branch (threads past the last word copy the last
// word again: the same value to the same address).
// LUT packed four bytes to a word: byte b = row offset of u = b (0 | 1..20 -> 48 | 21..46 -> 96 | 47..79 -> 144 | 80.. -> 192)
struct AtanTableImage { double rows[5][6]; unsigned lut[24]; };
static_assert(sizeof(AtanTableImage) == 8 * TPG_ATAN_TABLE_DOUBLES, "the image is the LDS table, word for word");
__device__ const AtanTableImage kAtanTable = {
    { { 1.0, 0.0, 1.0, 0.0, 0.0, 0.0 },                                        // [0, 0.4375): direct
      { 2.0, 1.0, 2.0, 1.0, 0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56 },     // [0.4375, 0.6875): (2x-1)/(2+x), atan(0.5)
      { 1.0, 1.0, 1.0, 1.0, 0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55 },     // [0.6875, 1.1875): (x-1)/(x+1),  atan(1)
      { 1.0, 1.5, 1.0, 1.5, 0x1.f730bd281f69bp-1, 0x1.007887af0cbbdp-56 },     // [1.1875, 2.4375): (x-1.5)/(1+1.5x), atan(1.5)
      { 0.0, 1.0, 0.0, 1.0, kPio2Hi, kPio2Lo } },                              // [2.4375, inf]:   -1/x, pi/2
    { 0x30303000u, 0x30303030u, 0x30303030u, 0x30303030u, 0x30303030u, 0x60606030u, 0x60606060u, 0x60606060u,
      0x60606060u, 0x60606060u, 0x60606060u, 0x90606060u, 0x90909090u, 0x90909090u, 0x90909090u, 0x90909090u,
      0x90909090u, 0x90909090u, 0x90909090u, 0x90909090u, 0xC0C0C0C0u, 0xC0C0C0C0u, 0xC0C0C0C0u, 0xC0C0C0C0u } };
// The copy in two halves, so that a kernel can issue the load first, do other work while it is in flight and store last.  tid >= 0.
TPG_DEV unsigned atan_table_word(int tid) { return (unsigned)tid < TPG_ATAN_TABLE_DOUBLES - 1u ? (unsigned)tid : TPG_ATAN_TABLE_DOUBLES - 1u; }
TPG_DEV unsigned long long atan_table_load(int tid)
{
    unsigned long long v;
    __builtin_memcpy(&v, reinterpret_cast<const char*>(&kAtanTable) + 8u * atan_table_word(tid), 8);
    return v;
}
TPG_DEV void atan_table_store(double* tab, int tid, unsigned long long v)
{
    __builtin_memcpy(reinterpret_cast<char*>(tab) + 8u * atan_table_word(tid), &v, 8);
}
TPG_DEV void atan_table_init(double* tab, int tid) { atan_table_store(tab, tid, atan_table_load(tid)); }

// atan(x), all x, with the interval constants taken from the LDS table (see atan_b for the
// value-equivalence of dropping the msun early-outs).  p = 0 on the last interval: the numerator
// uses min(ax, 2^1000) so that an infinite argument (y/x at x = +-0) still gives 0*ax - 1 = -1.
// FINITE = true: the caller guarantees finite arguments (e.g. sqrt(x^2 + y^2)) and the clamp is skipped.
// ABS = true: returns atan(|x|) = |atan(x)|, the value before the copysign: r = hi - ((t s - lo) - t) has its sign bit clear for every
// non-NaN x (hi >= 0.46 > |t| (1 + s) on the four reduced intervals; on the direct one r = 0 - (t s - t) with 0 <= t s <= t, and
// t = +0 gives 0 - ((0 - 0) - 0) = +0).  For callers that take |atan| anyway, or whose argument is never negative.
template <int N, bool FINITE = false, bool ABS = false> TPG_DEV void atan_tab_b(const double (&x)[N], double (&out)[N], const double* tab)
{
    double t[N], hi[N], lo[N], s[N];
#if defined(__HIP_DEVICE_COMPILE__)
    // the LUT's LDS address less the bias of u, as ONE scalar (the table is the wave's own): the clamp runs on the unbiased word and the
    // byte's address is one v_add_u32.  Left to itself the compiler adds the table's address first and the negative constant, which no
    // DS offset field can hold, second: two v_add_u32 per atan.
    typedef const unsigned char __attribute__((address_space(3))) lds_cbyte;
    unsigned lut0 = (unsigned)(uintptr_t)(lds_cbyte*)reinterpret_cast<const unsigned char*>(tab) + (8u * TPG_ATAN_ROWS_DOUBLES - 0x7FB7u);
    asm("" : "+s"(lut0));
#endif
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double ax = absD(x[e]);
#if defined(__HIP_DEVICE_COMPILE__)
        unsigned m = __builtin_amdgcn_ubfe((unsigned)__double2hiint(x[e]), 15u, 16u);               // bits 15..30 of the high word: sign dropped
        m = m < 0x7FB7u ? 0x7FB7u : (m > 0x7FB7u + 80u ? 0x7FB7u + 80u : m);
        const unsigned off = *(lds_cbyte*)(uintptr_t)(lut0 + m);                                     // bytes
#else
        int u = (int)__builtin_amdgcn_ubfe((unsigned)__double2hiint(x[e]), 15u, 16u) - 0x7FB7;     // bits 15..30 of the high word: sign dropped
        u = u < 0 ? 0 : (u > 80 ? 80 : u);
        const unsigned off = reinterpret_cast<const unsigned char*>(tab + TPG_ATAN_ROWS_DOUBLES)[u];   // bytes
#endif
        const AtanRow row = *reinterpret_cast<const AtanRow*>(reinterpret_cast<const char*>(tab) + off);
        hi[e] = row.hi; lo[e] = row.lo;
        const double axn = (!FINITE && ax > 0x1p1000) ? 0x1p1000 : ax;      // NaN stays NaN (and selects the direct row)
        const double num = row.p * axn - row.q;
        // den in [1, 1.5 * 2^1000] (axn, not ax: for ax >= 2^1000 the quotient -1/den is below 2^-999 either
        // way, its square underflows to 0 and hi - ((t*0 - lo) - t) rounds to hi - (-lo) regardless), so the
        // unscaled division is exact-equivalent; a NaN argument propagates through both forms
        const double den = row.r + row.s * axn;
        double q = tpgm::div_nr(num, den);
        asm volatile("" : "+v"(q));          // scheduling fence: keeps the live set of 4-wave kernels under 128 VGPRs
        t[e] = q;
    }
    {
        double z[N], w[N], s1[N], s2[N];
        TPG_UNROLL for (int e = 0; e < N; ++e) { z[e] = t[e] * t[e]; w[e] = z[e] * z[e]; }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], 1.62858201153657823623e-02, 4.97687799461593236017e-02);
                                                 s2[e] = fmaD(w[e], -3.65315727442169155270e-02, -5.83357013379057348645e-02); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 6.66107313738753120669e-02);
                                                 s2[e] = fmaD(w[e], s2[e], -7.69187620504482999495e-02); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 9.09088713343650656196e-02);
                                                 s2[e] = fmaD(w[e], s2[e], -1.11111104054623557880e-01); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 1.42857142725034663711e-01);
                                                 s2[e] = fmaD(w[e], s2[e], -1.99999999998764832476e-01); }
        TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 3.33333333333329318027e-01);
                                                 s2[e] = w[e] * s2[e]; }
        TPG_UNROLL for (int e = 0; e < N; ++e) s[e] = z[e] * s1[e] + s2[e];
    }
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double ts = t[e] * s[e];
        const double r = hi[e] - ((ts - lo[e]) - t[e]);
        out[e] = ABS ? r : csign(r, x[e]);
    }
}

// atan(x) for |x| < 0.4375: the msun "direct" branch only (no argument reduction, no division).
// The eight spherical-triangle tangents of a cell are O(cell area) ~ 1e-6, so this is their path.
// rare: some |x| >= 0.4375 (or NaN) -> caller uses atan_b.
// POS = true (the tile kernel's form): the fast path takes +0 <= x < 0.4375 only, as ONE unsigned compare of the high word (0.4375 has a
// zero low word; a set sign bit or a NaN's exponent make the word large), so it needs neither |x| nor the copysign of the result: t = x,
// and t - t s >= +0 is the result.  A negative tangent -- a triangle whose denominator 1 + a.b + b.c + a.c is negative: larger than a
// hemisphere -- is `rare` in this form and goes through atan_b, which gives the same bits (both equal tpgm::atanD).
template <int N, bool POS = false> TPG_DEV bool atan_small_b(const double (&x)[N], double (&out)[N])
{
    double t[N], z[N], w[N], s1[N], s2[N];
    bool rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        if (POS) { t[e] = x[e]; rare |= !((unsigned)__double2hiint(x[e]) < 0x3FDC0000u); }
        else     { t[e] = absD(x[e]); rare |= !(t[e] < 0.4375); }
    }
    TPG_UNROLL for (int e = 0; e < N; ++e) { z[e] = t[e] * t[e]; w[e] = z[e] * z[e]; }
    TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], 1.62858201153657823623e-02, 4.97687799461593236017e-02);
                                             s2[e] = fmaD(w[e], -3.65315727442169155270e-02, -5.83357013379057348645e-02); }
    TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 6.66107313738753120669e-02);
                                             s2[e] = fmaD(w[e], s2[e], -7.69187620504482999495e-02); }
    TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 9.09088713343650656196e-02);
                                             s2[e] = fmaD(w[e], s2[e], -1.11111104054623557880e-01); }
    TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 1.42857142725034663711e-01);
                                             s2[e] = fmaD(w[e], s2[e], -1.99999999998764832476e-01); }
    TPG_UNROLL for (int e = 0; e < N; ++e) { s1[e] = fmaD(w[e], s1[e], 3.33333333333329318027e-01);
                                             s2[e] = w[e] * s2[e]; }
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double sm = z[e] * s1[e] + s2[e];
        const double r = t[e] - t[e] * sm;
        out[e] = POS ? r : csign(r, x[e]);
    }
    return TPG_RARE(rare);
}

// atan(x) for +0 <= x < 2^-14: atan_small_b<N, true> with the Horner steps that are the identity there left out.  The tile kernel's first
// tier: on any grid finer than about 0.9 degrees every triangle tangent of a cell (~ a quarter of the cell's solid angle) lies below it.
// atan_small_b ends its two chains in w = t^4 with s1 = fma(w, s1', aT0), aT0 = 3.33333333333329318027e-01, and s2' = fma(w, s2'', aT1),
// aT1 = -1.99999999998764832476e-01.  fma(w, s, c) = RN(c + w s) is c whenever |w s| < ulp(c) / 2 and c is no power of two:
//   aT0 in [2^-2, 2^-1): half an ulp is 2^-55;  0 < s1' < 0.15 (a sum of positive terms, at most 0.1429 + w 0.091 + ...);
//   |aT1| in [2^-3, 2^-2): half an ulp is 2^-56;  |s2''| < 0.112;
//   t < 2^-14 gives w < 2^-56, so |w s1'| < 2^-58.7 and |w s2''| < 2^-59.1: margins of more than 2^3 on both.
// So s1 = aT0 and s2' = aT1 exactly, the eight fma in front of them are dead, and what is left -- z, w, s2 = w aT1, sm = z aT0 + s2,
// r = t - t sm, in atan_small_b's order -- has the bits of atan_small_b<N, true> (= tpgm::atanD): 7 operations per tangent for 16
// (tests/test_cells_atan_tiny.py: bit for bit on 10^6 random patterns, every power of two below 2^-14 and the last 10^5 doubles below it).
// rare: some x outside [+0, 2^-14), as ONE unsigned compare of the high word (2^-14 = 0x3F10000000000000 has a zero low word; a set sign
// bit, a NaN or an Inf make the word large) -> caller uses atan_small_b<N, true>, and its fallback behind that.
template <int N> TPG_DEV bool atan_tiny_b(const double (&x)[N], double (&out)[N])
{
    double z[N], w[N], s2[N];
    bool rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) rare |= !((unsigned)__double2hiint(x[e]) < 0x3F100000u);
    TPG_UNROLL for (int e = 0; e < N; ++e) { z[e] = x[e] * x[e]; w[e] = z[e] * z[e]; }
    TPG_UNROLL for (int e = 0; e < N; ++e) s2[e] = w[e] * -1.99999999998764832476e-01;
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double sm = z[e] * 3.33333333333329318027e-01 + s2[e];
        out[e] = x[e] - x[e] * sm;
    }
    return TPG_RARE(rare);
}

// asin(x) for |x| < 0.5.  tpgm::asinD returns x for |x| < 2^-26: x + x (p/q) with p/q ~ x^2/6
// rounds to x there.  rare: some |x| >= 0.5 (edges longer than 60 degrees: the overwritten row
// j = 1, toy grids) -> caller uses tpgm::asinD.
// asin_small_poly_b: the evaluation alone, for a caller that decides the domain by a test of its own (asin_sqrt_b below).
// SEEDLESS = true: for |x| < 2^-8 only.  q = 1 + t (qS1 + t (qS2 + ...)) with t = x^2 < 2^-16 and qS1 = -2.40339...: the inner sum lies
// in (-2.4034, -2.4033) (the next term is t qS2 < 2^-14.9), so q = 1 - d with 0 <= d < 2.41 * 2^-16 < 2^-14.73 after its rounding: the
// domain of tpgm::div_near<false>, which gives the bits of div_nr there without the v_rcp_f64.  Everything else is the same operation.
template <int N, bool SEEDLESS = false> TPG_DEV void asin_small_poly_b(const double (&x)[N], double (&out)[N])
{
    double t[N], p[N], q[N];
    TPG_UNROLL for (int e = 0; e < N; ++e) t[e] = x[e] * x[e];
    TPG_UNROLL for (int e = 0; e < N; ++e) { p[e] = fmaD(t[e], kc<N>(3.47933107596021167570e-05), kc<N>(7.91534994289814532176e-04));
                                             q[e] = fmaD(t[e], kc<N>(7.70381505559019352791e-02), kc<N>(-6.88283971605453293030e-01)); }
    TPG_UNROLL for (int e = 0; e < N; ++e) { p[e] = fmaD(t[e], p[e], kc<N>(-4.00555345006794114027e-02));
                                             q[e] = fmaD(t[e], q[e], kc<N>(2.02094576023350569471e+00)); }
    TPG_UNROLL for (int e = 0; e < N; ++e) { p[e] = fmaD(t[e], p[e], kc<N>(2.01212532134862925881e-01));
                                             q[e] = fmaD(t[e], q[e], kc<N>(-2.40339491173441421878e+00)); }
    TPG_UNROLL for (int e = 0; e < N; ++e) { p[e] = fmaD(t[e], p[e], kc<N>(-3.25565818622400915405e-01));
                                             q[e] = fmaD(t[e], q[e], 1.0); }
    TPG_UNROLL for (int e = 0; e < N; ++e) p[e] = fmaD(t[e], p[e], kc<N>(1.66666666666666657415e-01));
    TPG_UNROLL for (int e = 0; e < N; ++e) p[e] = t[e] * p[e];
    // q in (0.77, 1] for t < 0.25 and |p| <= 0.05 with p = 0 or |p| >= t/7 (t = x*x of a clamped sqrt: 0 or
    // >= 1e-40 here), so the unscaled division is exact-equivalent; lanes with |x| >= 0.5 or NaN are `rare`
    TPG_UNROLL for (int e = 0; e < N; ++e) out[e] = x[e] + x[e] * (SEEDLESS ? tpgm::div_near<false>(p[e], q[e]) : tpgm::div_nr(p[e], q[e]));
}
template <int N> TPG_DEV bool asin_small_b(const double (&x)[N], double (&out)[N])
{
    bool rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) rare |= !(absD(x[e]) < 0.5);
    asin_small_poly_b<N>(x, out);
    return TPG_RARE(rare);
}

// asin(min(sqrt(h), 1)), the tail of a haversine (h = 0 or >= ~1e-34: squares of half-differences of O(1) doubles), on the unscaled
// square root.  ONE test decides everything that derives from h: the unscaled square root of h = +-0 is NaN (rsq = +-Inf, 0 * Inf), of a
// NaN or a negative h as well, and r < 0.5 is false for a NaN.  So r < 0.5 says that h > 0 (sqrt_nr is in its domain), that min(r, 1) = r
// (no clamp) and that r lies in the fast domain of asin.  (Before: h == 0 with a patch of the square root, min(r, 1) as a v_min_f64 and
// asin_small_b's own |x| < 0.5 -- every element that took the patch or the scalar asin then fails the one test now.)
// The fallback evaluates the three as the reference has them: coincident points (pole-adjacent edges), edges longer than 60 degrees (the
// overwritten row j = 1, toy grids), NaN.
// A tier in front of that one, wave-uniform: r < 2^-8 on every element of every lane (edges shorter than 0.447 degrees: every haversine
// of a grid of 1/4 degree or finer away from its special rows) takes the polynomial with the seedless division of its p / q.  The compare
// stands where r < 0.5 stood, so the main path pays nothing for it; r < 2^-8 is false for what r < 0.5 is false for (NaN from h = +-0, a
// negative h or a NaN), and a wave with any such lane runs the code of before, test and all.  2^-8 is the largest power of two whose
// square keeps the denominator inside div_near's domain (2^-7: d < 2.41 * 2^-14).
// Returns whether the fallback ran (per lane).  tier, for the tests: 0 the seedless form (wave-uniform), 1 the polynomial with div_nr, 2 the
// fallback ran as well.
template <int N> TPG_DEV bool asin_sqrt_b(const double (&h)[N], double (&out)[N], int* tier = nullptr)
{
    double rt[N];
    bool far = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) { rt[e] = sqrt_nr<true>(h[e]); far |= TPG_RARE(!(rt[e] < 0x1p-8)); }
    if (!__any(far)) {
        asin_small_poly_b<N, true>(rt, out);
        if (tier) *tier = 0;
        return false;
    }
    bool rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) rare |= TPG_RARE(!(rt[e] < 0.5));
    asin_small_poly_b<N>(rt, out);
    if (rare) {
        TPG_UNROLL for (int e = 0; e < N; ++e) {
            const double r = sqrt_nr(h[e]);
            out[e] = asinD(!(r >= 1.0) ? r : 1.0);      // min(r, 1) that keeps a NaN, as the reference's
        }
    }
    if (tier) *tier = rare ? 2 : 1;
    return rare;
}

// a / b elementwise for denominators b = (1 - d) / c, c = 1 or 1/4 (QUARTER), through tpgm::div_near: the bits of div_nr without its
// v_rcp_f64.  The tile kernel's form for the four triangle denominators D = 1 + a.b + b.c + a.c of a quadrilateral, which are 4 (1 - d)
// with d ~ (sum of the three squared edge angles) / 8: 1.5e-6 at 1/10 degree, 1e-5 at 1/4 degree.
// rare: some element outside +0 <= d < 2^-16, read from the high words of the exact d = near_e(b) that the division starts from: the
// unsigned maximum of the N words against 0x3EF00000 (2^-16 has a zero low word) -- one v_max3_u32, one v_max_u32 and one compare for
// N = 4.  A NaN, an Inf or a b far from 1 / c make the word large, and so does every set sign bit: D exceeds 4 only by the rounding of a
// triangle whose three points all but coincide (d < 1e-16: edges below 3e-8 rad), which no ordinary cell has, so d < 0 is left to the
// caller's other form instead of paying for |d|; d = -0 does not occur (1 - 1 = +0).  -> caller uses div_nr.
template <int N, bool QUARTER> TPG_DEV bool div_near_b(const double (&a)[N], const double (&b)[N], double (&out)[N])
{
    const double c = tpgm::near_c<QUARTER>();
    unsigned m = 0u;
    TPG_UNROLL for (int e = 0; e < N; ++e) { const unsigned w = (unsigned)__double2hiint(tpgm::near_e(b[e], c)); m = w > m ? w : m; }
    TPG_UNROLL for (int e = 0; e < N; ++e) out[e] = tpgm::div_near(a[e], b[e], c);
    return TPG_RARE(!(m < 0x3EF00000u));
}

// sind / cosd pairs for |x| < 360 (longitudes in [0,360), latitudes in [-90,90]: rem(x,360) = x)
// One ladder of threshold compares serves both functions.  With m = the number of sind's thresholds (>= 45, > 135, >= 225, > 315)
// that r = |x| passes, d = 90 m - r, t = |d| and S = ksin, C = kcos of deg2rad(t):
//    sind = sign(x) * { +S, +C, sign(d) S, -C, -S }[m]
//    cosd =           { +C, sign(d) S, -C, (d > 0 ? -S : +S), +C }[m]
// cosd's own ladder (> 45, >= 135, > 225, >= 315) counts differently only AT a threshold, where m is odd, its own count is even
// and t = 45 for either: there cosd takes C, with the sign the table gives for sign(d) / d > 0 (r = 45: d = +45, +C; 135: d = -45,
// -C; 225: d = +45, -C; 315: d = -45, +C).  m = 3: cosd = sign(r - 270) S, and r - 270 = -d except that it is +0 where d = +0
// (r = 270, cosd = +0), hence "d > 0" and not the sign bit; d is never -0 (a difference of equal numbers is +0).
// The factors +-1 are applied as an xor on the high word: x * +-1.0 is exact and only sets the sign (of a zero as well), so the bits
// are those of the product for every non-NaN x.  All of it is checked bit for bit against the two-ladder form it replaces:
// tests/test_cells_trims.py.
// POS = true: the caller guarantees that no x has its sign bit set (the longitudes of the tile kernel, which leave fmod360_pos).
template <int N, bool POS = false> TPG_DEV void sincosd_b(const double (&x)[N], double (&sn)[N], double (&cs)[N])
{
    double h[N], l[N], S[N], C[N];
    bool sC[N], cS[N];           // sind takes C / cosd takes S
    int ws[N], wc[N];            // bit 31: sind / cosd is negated
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double r = absD(x[e]);
        const bool s1 = r >= 45.0, s2 = r > 135.0, s3 = r >= 225.0, s4 = r > 315.0;
        int mh = 0;                                                        // high word of 90 m (the low words are zero)
        mh = s1 ? 0x40568000 : mh; mh = s2 ? 0x40668000 : mh; mh = s3 ? 0x4070E000 : mh; mh = s4 ? 0x40768000 : mh;
        const double d = __hiloint2double(mh, 0) - r;
        const double t = absD(d);
        const double hh = t * kDeg2Rad;
        l[e] = fmaD(t, kDeg2Rad, -hh) + t * kDeg2RadLo;
        h[e] = hh;
        const int dh = __double2hiint(d);
        const bool odd = (s1 != s2) != (s3 != s4), m1 = s1 && !s2, m2 = s2 && !s3, m3 = s3 && !s4;
        sC[e] = odd;
        cS[e] = odd && t != 45.0;
        const int sneg = s3 ? (int)0x80000000 : 0;
        ws[e] = m2 ? dh : sneg;
        const int cneg = (m2 || (m3 && d > 0.0)) ? (int)0x80000000 : 0;
        wc[e] = m1 ? dh : cneg;
        if (!POS) ws[e] ^= __double2hiint(x[e]);
    }
    ksin_b<N>(h, l, S);
    kcos_b<N>(h, l, C);
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const int slo = sC[e] ? __double2loint(C[e]) : __double2loint(S[e]), shi = sC[e] ? __double2hiint(C[e]) : __double2hiint(S[e]);
        const int clo = cS[e] ? __double2loint(S[e]) : __double2loint(C[e]), chi = cS[e] ? __double2hiint(S[e]) : __double2hiint(C[e]);
        sn[e] = __hiloint2double(shi ^ (ws[e] & (int)0x80000000), slo);
        cs[e] = __hiloint2double(chi ^ (wc[e] & (int)0x80000000), clo);
    }
}

// sind / cosd pairs for latitudes, |x| <= 90: of sincosd_b's eight octant compares only the first of each set can be true, 90 m is
// 0 or 90, the sine carries the sign of x and the cosine is never negated (90 - r >= +0):
//    r < 45 (sind) / r <= 45 (cosd):  sind = sign(x) ksin(r),        cosd = kcos(r)
//    otherwise:                        sind = sign(x) kcos(90 - r),   cosd = ksin(90 - r)
// -- the same reduction t = |90 m - r|, the same kernels and therefore the same bits as sincosd_b / tpgm::sind, cosd.
// rare: some |x| > 90 or NaN -> caller uses sincosd_b.
template <int N> TPG_DEV bool sincosd_lat_b(const double (&x)[N], double (&sn)[N], double (&cs)[N])
{
    double h[N], l[N], S[N], C[N];
    bool s1[N], c1[N], rare = false;
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double r = absD(x[e]);
        rare |= !(r <= 90.0);
        s1[e] = r >= 45.0; c1[e] = r > 45.0;
        const double d = (s1[e] ? 90.0 : 0.0) - r;
        const double t = absD(d);
        const double hh = t * kDeg2Rad;
        l[e] = fmaD(t, kDeg2Rad, -hh) + t * kDeg2RadLo;
        h[e] = hh;
    }
    ksin_b<N>(h, l, S);
    kcos_b<N>(h, l, C);
    TPG_UNROLL for (int e = 0; e < N; ++e) {
        const double bs = s1[e] ? C[e] : S[e];
        // sign(x) * bs as a copysign: bs = ksin / kcos of deg2rad(t), 0 <= t <= 45, has its sign bit clear (ksin(+0, +0) = +0), and the
        // product with +-1.0 is exact -- it sets the sign and nothing else.  (|x| > 90 or NaN: `rare`, the caller discards this)
        sn[e] = csign(bs, x[e]);
        cs[e] = c1[e] ? S[e] : C[e];
    }
    return TPG_RARE(rare);
}

// fmod(x, 360) for 0 <= x < 720 (the second application in ((l % 360) + 360) % 360: l % 360 is in (-360, 360))
TPG_DEV double fmod360_pos(double x)
{
    // x - (x >= 360 ? 360 : 0): both constants have a zero low word, so the select is ONE v_cndmask on the high word, and x - 0.0 = x
    // for every x (signed zeros included)
    return x - __hiloint2double(!(x < 360.0) ? 0x40768000 : 0, 0);
}

// exact fmod(x, 360) for |x| < 720 (select form of tpgm::fmod360)
TPG_DEV double fmod360_small(double x)
{
    const double ax = absD(x);
    return csign(ax - __hiloint2double(!(ax < 360.0) ? 0x40768000 : 0, 0), x);       // csign(|x| - 0, x) = x
}

}  // namespace tpgb
