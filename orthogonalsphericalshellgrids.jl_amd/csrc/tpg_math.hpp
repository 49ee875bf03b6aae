// tpg_math.hpp -- deterministic Float64 elementary functions for gfx950 device code.
//
// The TripolarGrid metric precompute must agree with the CPU reference path to <= 1e-12
// relative on Float64 metrics (BASELINE.json north_star).  Edge lengths are haversines of
// *differences* of O(100 deg) coordinates, so a 1-ulp coordinate discrepancy already costs
// ~5e-13 at 1/10 deg ("Conditioning").  OCML's sin/cos/atan/asin are not
// bit-compatible with any host libm, therefore every transcendental used on the path is built
// here from IEEE-754 correctly rounded primitives only (+ - * / sqrt fma rint, bit ops): the same
// operation sequence gives the same bits on any IEEE machine.  Must be compiled with
// -ffp-contract=off (fusions are explicit __builtin_fma).
//
// Algorithms: FreeBSD msun family (k_sin, k_cos, e_rem_pio2 medium path, s_atan, e_asin) -- the
// algorithms Julia Base ports for sin/cos/atan/asin -- plus Julia-style degree-exact sind/cosd
// (exact rem(x,360) reduction, octant selection, double-double deg->rad product), and a
// double-double exp/log for the O(Ny) latitude-stretching table (asinh, sinh, cosh).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpgm {

#define TPG_DEV __device__ __forceinline__

constexpr double kPi       = 0x1.921fb54442d18p+1;
constexpr double kDeg2Rad  = 0x1.1df46a2529d39p-6;    // Float64(pi)/180  (Julia deg2rad)
constexpr double kDeg2RadLo = 0x1.5c1d8becdd291p-62;  // pi/180 - kDeg2Rad
constexpr double kInvPio2  = 0x1.45f306dc9c883p-1;
constexpr double kPio2_1   = 0x1.921fb54400000p+0;
constexpr double kPio2_1t  = 0x1.0b4611a626331p-34;
constexpr double kPio2_2   = 0x1.0b4611a600000p-34;
constexpr double kPio2_2t  = 0x1.3198a2e037073p-69;
constexpr double kPio2_3   = 0x1.3198a2e000000p-69;
constexpr double kPio2_3t  = 0x1.b839a252049c1p-104;
constexpr double kPio2Hi   = 0x1.921fb54442d18p+0;
constexpr double kPio2Lo   = 0x1.1a62633145c07p-54;
constexpr double kPio4Hi   = 0x1.921fb54442d18p-1;
constexpr double kLn2Hi    = 0x1.62e42fefa39efp-1;
constexpr double kLn2Lo    = 0x1.abc9e3b39803fp-56;

TPG_DEV uint64_t bits(double x) { return (uint64_t)__double_as_longlong(x); }
TPG_DEV double from_bits(uint64_t u) { return __longlong_as_double((long long)u); }
TPG_DEV int expo(double x) { return (int)((bits(x) >> 52) & 0x7ff); }
TPG_DEV double fmaD(double a, double b, double c) { return __builtin_fma(a, b, c); }
TPG_DEV double absD(double x) { return __builtin_fabs(x); }

// a / b and sqrt(x) WITHOUT the range scaling and special-case fix-up of the compiler's expansions
// (v_div_scale x2 + v_div_fixup; v_cmp/v_ldexp x2 + v_cmp_class/v_cndmask): the same Newton-Raphson
// sequence on v_rcp_f64 / v_rsq_f64 that those expansions wrap, so the result is bit-identical to the
// IEEE operation whenever the wrapper would not have acted:
//   div_nr : b finite, 2^-1000 <= |b| <= 2^1000, a = 0 or a/b comfortably normal (callers document why)
//   sqrt_nr: x = +-0, or 2^-767 <= x < inf  (x = 0 is handled by one select; NaN propagates)
// 8 instead of 11 instructions per division, 13 instead of ~20 per square root -- ~6 % of the cell
// kernel's VALU work.  Callers that cannot bound their operands keep `/` and sqrt().
TPG_DEV double div_nr(double a, double b)
{
    double r = __builtin_amdgcn_rcp(b);
    double e = fmaD(-b, r, 1.0);
    r = fmaD(r, e, r);
    e = fmaD(-b, r, 1.0);
    r = fmaD(r, e, r);
    const double q = a * r;
    e = fmaD(-b, q, a);
    return fmaD(e, r, q);
}
// a / b for a denominator next to a known constant: b = (1 - d) / c with c = 1 (QUARTER = false) or c = 1/4 (QUARTER = true) and
// |d| < 2^-14.  div_nr from its first `e` onward with r = c in the place of v_rcp_f64(b): the same seven operations, no seed instruction
// (which costs 3.3-3.4 plain Float64 instructions, profiles/HISTORY.md).  near_e is that first e, which a caller's tier test reads.
//   e0 = fma(-b, c, 1) = 1 - b c = d EXACTLY: b c is b scaled by a power of two, it lies within [1 - 2^-14, 1 + 2^-14], and the
//        difference of two doubles within a factor of two of each other is a double (Sterbenz); the fma rounds once, to that double.
//   r1 = fma(c, e0, c) = RN(c (1 + d)).  1 / b = c / (1 - d) = c (1 + d) / (1 - d^2), so r1 = (1 - d^2)(1 + p1) / b, |p1| <= 2^-53:
//        relative error e1 = 1 - b r1 with |e1| <= d^2 + 2^-53 < 2^-27.99.
//   e  = fma(-b, r1, 1) = RN(e1) (relative rounding error 2^-53 of a number below 2^-27.99: below 2^-81 absolute);
//   r2 = fma(r1, e, r1) = RN(r1 (1 + e)) = (1 - e1^2)(1 + p2) / b up to that 2^-81: r2 = (1 + n) / b with
//        |n| <= 2^-53 + e1^2 + 2^-80 and e1^2 <= (d^2 + 2^-53)^2 < d^4 + 2^-79.
//        |d| < 2^-14: d^4 < 2^-56, an eighth of r2's own rounding error 2^-53 (the factor atan_tiny_b keeps as well).  2^-13 would leave
//        2^-52, twice the rounding error: 2^-14 is the largest power of two with a margin at all.  The two callers stay further inside:
//        the triangle denominators test |d| < 2^-16 (d^4 < 2^-64, a margin of 2^11) and the asin tail has |d| < 2.41 * 2^-16 < 2^-14.73
//        (d^4 < 2^-58.9, a margin of 2^5.9).
//   q0 = RN(a r2);  e2 = fma(-b, q0, a) = a - b q0 EXACTLY (the residual of a quotient that is within an ulp of a / b is a double);
//   q  = RN(q0 + e2 r2) = RN(a / b + (e2 / b) n): the last step adds the exact residual over b, whatever q0 was, so it depends on the
//        seed only through n, and |e2 / b| <= ulp(q0) puts the value that is rounded within |n| ulp -- 2^-52.8 of an ulp -- of a / b.
//        That is the state div_nr reaches from the hardware seed (its r carries the same half ulp of its last rounding), and like div_nr
//        the form is HELD to the bits of IEEE a / b on its range by test, not proved correctly rounded for every pair: a / b would have
//        to lie within 2^-52.8 ulp of a rounding boundary to differ.  tests/test_cells_seedless_div.py: 10^7 random pairs per form over
//        the whole of |d| < 2^-14, every power of two of d with its neighbours, the last 10^5 doubles below the threshold, b = 1 / c and
//        its neighbours, a = +0, against IEEE `/` and against div_nr; on the device against div_nr through the math probe.
// a: as for div_nr (a = +0, or a / b comfortably normal; a = -0 gives +0 through both: e2 = (+0) + (-0) = +0).  NaN and Inf propagate as through div_nr, but no caller sends them here.
// near_c: the constant c.  1/4 is no inline constant of the Float64 instructions and would be built in a vector register pair at every
// use (two v_mov_b32 per division); pinned to a scalar pair once per caller, the fma reads it as its one scalar operand (cf. tpgb::kc).
template <bool QUARTER> TPG_DEV double near_c()
{
    double c = QUARTER ? 0.25 : 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
    if (QUARTER) asm("" : "+s"(c));
#endif
    return c;
}
TPG_DEV double near_e(double b, double c) { return fmaD(-b, c, 1.0); }
TPG_DEV double div_near(double a, double b, double c)
{
    double e = near_e(b, c);
    double r = fmaD(c, e, c);
    e = fmaD(-b, r, 1.0);
    r = fmaD(r, e, r);
    const double q = a * r;
    e = fmaD(-b, q, a);
    return fmaD(e, r, q);
}
template <bool QUARTER> TPG_DEV double div_near(double a, double b) { return div_near(a, b, near_c<QUARTER>()); }
// NONZERO = true: the caller guarantees x > 0 (no select for the zero case)
template <bool NONZERO = false> TPG_DEV double sqrt_nr(double x)
{
    const double r = __builtin_amdgcn_rsq(x);
    double g = x * r;
    double h = r * 0.5;
    const double e = fmaD(-h, g, 0.5);
    g = fmaD(g, e, g);
    double d = fmaD(-g, g, x);
    h = fmaD(h, e, h);
    g = fmaD(d, h, g);
    d = fmaD(-g, g, x);
    g = fmaD(d, h, g);
    return (!NONZERO && x == 0.0) ? x : g;
}
TPG_DEV double csign(double mag, double sgn) { return __builtin_copysign(mag, sgn); }

// exact fmod(x, 360): identity / one exact subtraction (Sterbenz) on the ranges the grid uses,
// generic exact remainder otherwise.
TPG_DEV double fmod360(double x)
{
    double ax = absD(x);
    if (ax < 360.0) return x;
    if (ax < 720.0) return csign(ax - 360.0, x);
    return fmod(x, 360.0);
}

// ---- kernels on [-pi/4, pi/4], argument x + y (double-double)
TPG_DEV double ksin(double x, double y)
{
    double z = x * x;
    double r = fmaD(z, fmaD(z, fmaD(z, fmaD(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                    2.75573137070700676789e-06), -1.98412698298579493134e-04),
                    8.33333333332248946124e-03);
    double v = z * x;
    return x - ((z * (0.5 * y - v * r) - y) - v * -1.66666666666666324348e-01);
}
TPG_DEV double kcos(double x, double y)
{
    double z = x * x;
    double r = z * fmaD(z, fmaD(z, fmaD(z, fmaD(z, fmaD(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                            -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                                -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    double hz = 0.5 * z;
    double w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + (z * r - x * y));
}

// ---- Cody-Waite reduction by pi/2 (|x| < 2^20 pi/2)
TPG_DEV int rem_pio2(double x, double& y0, double& y1)
{
    double fn = __builtin_rint(x * kInvPio2);
    int n = (int)fn;
    double r = x - fn * kPio2_1;
    double w = fn * kPio2_1t;
    int j = expo(x);
    double a = r - w;
    if (j - expo(a) > 16) {
        double t = r;
        w = fn * kPio2_2;
        r = t - w;
        w = fn * kPio2_2t - ((t - r) - w);
        a = r - w;
        if (j - expo(a) > 49) {
            t = r;
            w = fn * kPio2_3;
            r = t - w;
            w = fn * kPio2_3t - ((t - r) - w);
            a = r - w;
        }
    }
    y0 = a;
    y1 = (r - a) - w;
    return n;
}

// sin and cos of the same radian argument (haversine needs both kinds on different arguments;
// sharing the reduction is free determinism-wise: each output equals the scalar function)
TPG_DEV double sinD(double x)
{
    if (!(absD(x) <= kPio4Hi)) {
        double y0, y1;
        int n = rem_pio2(x, y0, y1);
        double s = ksin(y0, y1), c = kcos(y0, y1);
        double v = (n & 1) ? c : s;
        return (n & 2) ? -v : v;
    }
    if (expo(x) < 0x3e5) return x;
    return ksin(x, 0.0);
}
TPG_DEV double cosD(double x)
{
    if (!(absD(x) <= kPio4Hi)) {
        double y0, y1;
        int n = rem_pio2(x, y0, y1);
        double s = ksin(y0, y1), c = kcos(y0, y1);
        double v = (n & 1) ? s : c;
        return ((n + 1) & 2) ? -v : v;
    }
    return kcos(x, 0.0);
}

// ---- degree trig
TPG_DEV void deg2rad_ext(double x, double& hi, double& lo)
{
    double h = x * kDeg2Rad;
    lo = fmaD(x, kDeg2Rad, -h) + x * kDeg2RadLo;
    hi = h;
}
TPG_DEV double sind(double x)
{
    double rx = csign(fmod360(x), x);
    double arx = absD(rx);
    if (rx == 0.0) return rx;
    if (arx == 180.0) return csign(0.0, rx);
    double arg, sg;
    bool use_cos, neg = false;
    if (arx < 45.0)        { arg = rx; use_cos = false; sg = 0.0; }
    else if (arx <= 135.0) { arg = 90.0 - arx; use_cos = true; sg = rx; }
    else if (arx < 225.0)  { arg = (180.0 - arx) * csign(1.0, rx); use_cos = false; sg = 0.0; }
    else if (arx <= 315.0) { arg = 270.0 - arx; use_cos = true; sg = rx; neg = true; }
    else                   { arg = rx - csign(360.0, rx); use_cos = false; sg = 0.0; }
    double h, l;
    deg2rad_ext(arg, h, l);
    if (use_cos) {
        double c = csign(kcos(h, l), sg);
        return neg ? -c : c;
    }
    return ksin(h, l);
}
TPG_DEV double cosd(double x)
{
    double rx = absD(fmod360(x));
    double arg;
    bool use_sin, neg = false;
    if (rx <= 45.0)       { arg = rx; use_sin = false; }
    else if (rx < 135.0)  { arg = 90.0 - rx; use_sin = true; }
    else if (rx <= 225.0) { arg = 180.0 - rx; use_sin = false; neg = true; }
    else if (rx < 315.0)  { arg = rx - 270.0; use_sin = true; }
    else                  { arg = 360.0 - rx; use_sin = false; }
    double h, l;
    deg2rad_ext(arg, h, l);
    if (use_sin) return ksin(h, l);
    double c = kcos(h, l);
    return neg ? -c : c;
}

// sind(x) and cosd(x) together: both functions reduce x to the same distance t from the nearest
// multiple of 90 (ties at 45+90k give t = 45 either way) and evaluate the sin- or cos-kernel on the
// same double-double radian argument, so one reduction + one ksin + one kcos yields both values with
// exactly the bits sind() and cosd() return separately (ksin is odd, kcos even, deg2rad_ext odd --
// all exactly).
TPG_DEV void sincosd(double x, double& sn, double& cs)
{
    double rx = csign(fmod360(x), x);
    double r = absD(rx);
    double sg = csign(1.0, rx);
    // nearest multiple of 90 for sind (ties -> 90/270) and for cosd (ties -> 0/180/360)
    int ms = r < 45.0 ? 0 : (r <= 135.0 ? 1 : (r < 225.0 ? 2 : (r <= 315.0 ? 3 : 4)));
    int mc = r <= 45.0 ? 0 : (r < 135.0 ? 1 : (r <= 225.0 ? 2 : (r < 315.0 ? 3 : 4)));
    double d = (double)(90 * ms) - r;                 // signed offset to sind's multiple
    double t = absD(d);                                // == |90*mc - r| as well
    double h, l;
    deg2rad_ext(t, h, l);
    double S = ksin(h, l), C = kcos(h, l);
    double dsg = csign(1.0, d);                        // sign(90*ms - r)
    switch (ms) {
    case 0:  sn = sg * S; break;                       // ksin(d2r(rx))
    case 1:  sn = sg * C; break;                       // copysign(kcos(d2r(90-r)), rx)
    case 2:  sn = (dsg * sg) * S; break;               // ksin(d2r((180-r)*sign(rx))); r == 180 -> +-0
    case 3:  sn = -(sg * C); break;                    // -copysign(kcos(d2r(270-r)), rx)
    default: sn = -(sg * S); break;                    // ksin(d2r(rx - copysign(360, rx)))
    }
    switch (mc) {
    case 0:  cs = C; break;                            // kcos(d2r(r))
    case 1:  cs = csign(1.0, 90.0 - r) * S; break;     // ksin(d2r(90-r))   (+0 at r = 90)
    case 2:  cs = -C; break;                           // -kcos(d2r(180-r))
    case 3:  cs = csign(1.0, r - 270.0) * S; break;    // ksin(d2r(r-270))  (+0 at r = 270)
    default: cs = C; break;                            // kcos(d2r(360-r))
    }
}
TPG_DEV double tand(double x) { return sind(x) / cosd(x); }

// ---- atan
TPG_DEV double atanD(double x)
{
    double ax = absD(x);
    if (x != x) return x;
    if (ax >= 0x1p66) return csign(kPio2Hi + kPio2Lo, x);
    if (ax < 0x1p-27) return x;
    double num, den, hi, lo;
    bool direct = ax < 0.4375;
    if (ax < 0.6875)      { num = 2.0 * ax - 1.0; den = 2.0 + ax;       hi = 0x1.dac670561bb4fp-2; lo = 0x1.a2b7f222f65e2p-56; }
    else if (ax < 1.1875) { num = ax - 1.0;       den = ax + 1.0;       hi = 0x1.921fb54442d18p-1; lo = 0x1.1a62633145c07p-55; }
    else if (ax < 2.4375) { num = ax - 1.5;       den = 1.0 + 1.5 * ax; hi = 0x1.f730bd281f69bp-1; lo = 0x1.007887af0cbbdp-56; }
    else                  { num = -1.0;           den = ax;             hi = kPio2Hi;              lo = kPio2Lo; }
    double t = direct ? ax : num / den;
    double z = t * t;
    double w = z * z;
    double s1 = z * fmaD(w, fmaD(w, fmaD(w, fmaD(w, fmaD(w, 1.62858201153657823623e-02, 4.97687799461593236017e-02),
                                              6.66107313738753120669e-02), 9.09088713343650656196e-02),
                                  1.42857142725034663711e-01), 3.33333333333329318027e-01);
    double s2 = w * fmaD(w, fmaD(w, fmaD(w, fmaD(w, -3.65315727442169155270e-02, -5.83357013379057348645e-02),
                                      -7.69187620504482999495e-02), -1.11111104054623557880e-01),
                          -1.99999999998764832476e-01);
    double r = direct ? t - t * (s1 + s2) : hi - ((t * (s1 + s2) - lo) - t);
    return csign(r, x);
}

// ---- asin
TPG_DEV double asin_pq(double t)
{
    double p = t * fmaD(t, fmaD(t, fmaD(t, fmaD(t, fmaD(t, 3.47933107596021167570e-05, 7.91534994289814532176e-04),
                                            -4.00555345006794114027e-02), 2.01212532134862925881e-01),
                                -3.25565818622400915405e-01), 1.66666666666666657415e-01);
    double q = fmaD(t, fmaD(t, fmaD(t, fmaD(t, 7.70381505559019352791e-02, -6.88283971605453293030e-01),
                                    2.02094576023350569471e+00), -2.40339491173441421878e+00), 1.0);
    return p / q;
}
TPG_DEV double asinD(double x)
{
    double ax = absD(x);
    if (ax >= 1.0) {
        if (ax == 1.0) return x * kPio2Hi + x * kPio2Lo;
        return (x - x) / (x - x);
    }
    if (ax < 0.5) {
        if (ax < 0x1p-26) return x;
        return x + x * asin_pq(x * x);
    }
    double w = 1.0 - ax;
    double t = w * 0.5;
    double r = asin_pq(t);
    double s = sqrt(t);
    double res;
    if (ax >= 0.975) {
        res = kPio2Hi - (2.0 * (s + s * r) - kPio2Lo);
    } else {
        double f = from_bits(bits(s) & 0xffffffff00000000ull);
        double c = (t - f * f) / (s + f);
        double p = 2.0 * s * r - (kPio2Lo - 2.0 * c);
        double q = kPio4Hi - 2.0 * f;
        res = kPio4Hi - (p - q);
    }
    return csign(res, x);
}

// ---- acos (msun e_acos.c; the same p/q as asin) -- used by the non-orthogonality diagnostic only
TPG_DEV double acosD(double x)
{
    double ax = absD(x);
    if (ax >= 1.0) {
        if (ax == 1.0) return x > 0.0 ? 0.0 : kPi;
        return (x - x) / (x - x);
    }
    if (ax < 0.5) {
        if (ax < 0x1p-54) return kPio2Hi;                          // eps/4: pi/2 to the last bit
        double z = x * x;
        return kPio2Hi - (x - (kPio2Lo - x * asin_pq(z)));
    }
    double z = (1.0 - ax) * 0.5;
    double r = asin_pq(z);
    double s = sqrt(z);
    if (x < 0.0) return kPi - 2.0 * (s + (r * s - kPio2Lo));
    double f = from_bits(bits(s) & 0xffffffff00000000ull);
    double c = (z - f * f) / (s + f);
    return 2.0 * (f + (r * s + c));
}

// ---- double-double toolkit (latitude-stretching table only)
struct dd { double hi, lo; };
TPG_DEV dd two_sum(double a, double b) { double s = a + b, bb = s - a; return { s, (a - (s - bb)) + (b - bb) }; }
TPG_DEV dd quick_two_sum(double a, double b) { double s = a + b; return { s, b - (s - a) }; }
TPG_DEV dd two_prod(double a, double b) { double p = a * b; return { p, fmaD(a, b, -p) }; }
TPG_DEV dd dd_add(dd a, dd b)
{
    dd s = two_sum(a.hi, b.hi), t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return quick_two_sum(s.hi, s.lo);
}
TPG_DEV dd dd_neg(dd a) { return { -a.hi, -a.lo }; }
TPG_DEV dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
TPG_DEV dd dd_mul(dd a, dd b)
{
    dd p = two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return quick_two_sum(p.hi, p.lo);
}
TPG_DEV dd dd_mul_d(dd a, double b)
{
    dd p = two_prod(a.hi, b);
    p.lo += a.lo * b;
    return quick_two_sum(p.hi, p.lo);
}
TPG_DEV dd dd_div(dd a, dd b)
{
    double q1 = a.hi / b.hi;
    dd r = dd_sub(a, dd_mul_d(b, q1));
    double q2 = r.hi / b.hi;
    r = dd_sub(r, dd_mul_d(b, q2));
    double q3 = r.hi / b.hi;
    dd q = quick_two_sum(q1, q2);
    return dd_add(q, dd{ q3, 0.0 });
}
TPG_DEV dd dd_sqrt(dd a)
{
    if (a.hi <= 0.0) return { 0.0, 0.0 };
    double x = 1.0 / sqrt(a.hi);
    double ax = a.hi * x;
    dd e = dd_sub(a, two_prod(ax, ax));
    return two_sum(ax, e.hi * (x * 0.5));
}
__device__ __noinline__ dd dd_expm1_reduced(dd a, int& kout)
{
    const dd ln2 = { kLn2Hi, kLn2Lo };
    double kf = __builtin_rint(a.hi / kLn2Hi);
    dd r = dd_sub(a, dd_mul_d(ln2, kf));
    r.hi *= 0x1p-9; r.lo *= 0x1p-9;
    // Taylor to r^11/11!, Horner in double-double: s = r + r^2 (1/2! + r (1/3! + ...))
    const dd invfact[10] = {
    { 0x1.0000000000000p-1, 0x0.0p+0 },                // 1/2! 
    { 0x1.5555555555555p-3, 0x1.5555555555555p-57 },   // 1/3! 
    { 0x1.5555555555555p-5, 0x1.5555555555555p-59 },   // 1/4! 
    { 0x1.1111111111111p-7, 0x1.1111111111111p-63 },   // 1/5! 
    { 0x1.6c16c16c16c17p-10, -0x1.f49f49f49f49fp-65 }, // 1/6! 
    { 0x1.a01a01a01a01ap-13, 0x1.a01a01a01a01ap-73 },  // 1/7! 
    { 0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76 },  // 1/8! 
    { 0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73 }, // 1/9! 
    { 0x1.27e4fb7789f5cp-22, 0x1.cbbc05b4fa99ap-76 },  // 1/10!
    { 0x1.ae64567f544e4p-26, -0x1.c062e06d1f209p-80 }, // 1/11!
    };
    dd pl = invfact[9];
    for (int n = 8; n >= 0; --n) pl = dd_add(invfact[n], dd_mul(r, pl));
    dd s = dd_add(r, dd_mul(dd_mul(r, r), pl));
    for (int i = 0; i < 9; ++i) s = dd_add(dd_mul_d(s, 2.0), dd_mul(s, s));
    kout = (int)kf;
    return s;
}
TPG_DEV dd dd_exp(dd a)
{
    int k;
    dd s = dd_expm1_reduced(a, k);
    dd e = dd_add(dd{ 1.0, 0.0 }, s);
    double sc = from_bits((uint64_t)(1023 + k) << 52);
    e.hi *= sc; e.lo *= sc;
    return e;
}
TPG_DEV dd dd_log(dd a)
{
    int e = expo(a.hi) - 1023;
    double m = from_bits((bits(a.hi) & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    if (m > 0x1.6a09e667f3bcdp+0) { m *= 0.5; e += 1; }
    double u = (m - 1.0) / (m + 1.0), u2 = u * u;
    double ser = u * (2.0 + u2 * (2.0 / 3.0 + u2 * (2.0 / 5.0 + u2 * (2.0 / 7.0 + u2 * (2.0 / 9.0
                 + u2 * (2.0 / 11.0 + u2 * (2.0 / 13.0 + u2 * (2.0 / 15.0 + u2 * (2.0 / 17.0 + u2 * (2.0 / 19.0))))))))));
    dd y = two_sum((double)e * kLn2Hi, ser);
    for (int it = 0; it < 1; ++it) {       // seed ~3e-16 -> ~5e-32: one Newton step reaches the double-double floor
        dd ey = dd_exp(dd_neg(y));
        dd c = dd_sub(dd_mul(a, ey), dd{ 1.0, 0.0 });
        y = dd_add(y, c);
    }
    return y;
}
TPG_DEV double asinhD(double x)
{
    double ax = absD(x);
    if (ax == 0.0 || x != x) return x;
    dd s = dd_sqrt(dd_add(two_prod(ax, ax), dd{ 1.0, 0.0 }));
    dd l = dd_log(dd_add(dd{ ax, 0.0 }, s));
    return csign(l.hi + l.lo, x);
}
TPG_DEV void sinh_cosh(double x, double& sh, double& ch)
{
    double ax = absD(x);
    dd e = dd_exp(dd{ ax, 0.0 });
    dd ie = dd_div(dd{ 1.0, 0.0 }, e);
    dd s = dd_sub(e, ie), c = dd_add(e, ie);
    sh = csign(0.5 * (s.hi + s.lo), x);
    ch = 0.5 * (c.hi + c.lo);
}

}  // namespace tpgm
