// tpg_grid.hip -- TripolarGrid coordinate + staggered-metric precompute for gfx950.
//
// Replaces src/tripolar_grid.jl:73-328 of the reference (see include/tripolar_hip.h).  The
// reference runs ~40 full-array host passes (two CPU KernelAbstractions kernels, 8 circshifts,
// 20 Field set!/fill_halo_regions!/deepcopy round trips, 12 continue_south!, 20 map+H2D copies);
// here the final padded device arrays are produced directly by four launches on one stream:
//
//   K0 tables      : per-i  a*sind(lambda), a*cosd(lambda) (Face, Center; the Nlambda/4 circshift is
//                    folded into the index), per-j sinh(psi), cosh(psi) latitude-stretching tables
//                    (Face, Center), and the (Hy+1)-row lat-lon continuation table.  O(Nx+Ny) work.
//   K1 cells       : every interior cell (i, j) of the rank's row band: the Murray (1996) map at the 4
//                    staggered locations of the cell and of its stencil neighbours THROUGH the halo
//                    index maps (periodic x, zipper fold, row-Ny substitution, zero south halo),
//                    then the 8 haversine edge lengths, 2 spherical quadrilateral areas and 2
//                    product areas; stores 8 + 12 values.  Two forms with identical arithmetic
//                    (tests/test_gpu_variants.py), selected by TPG_CELLS_VARIANT:
//                      2  k_cells_tile   DEFAULT, the product's only form (blocks take their tiles in an XCD-grouped order, see
//                                        tile_of_block).  A block of 8 waves evaluates 8 point rows x 64
//                                        columns once (one point set per thread), parks them in LDS
//                                        and, after one barrier, every thread computes its cell from
//                                        its own registers + LDS neighbours.  <= 128 VGPRs: 4
//                                        waves/SIMD; transcendentals as straight-line batches
//                                        (tpg_batch.hpp).  A wave's 64 columns are two strips of 32 that
//                                        are lambda -> -lambda images of each other: the latitude / atan
//                                        chain of a point is evaluated by one lane of the pair and handed
//                                        to the other through LDS (points_pair).
//                      0  k_cells        one thread per cell, everything recomputed: the simple
//                                        reference form the tile kernel is checked against.
//                    (Round 1 also carried two register-marching forms -- waves of 62 columns marching
//                    north with the previous row in registers, 256 VGPRs, 2 waves/SIMD: 664-706 us vs the
//                    tile form's 499 us at 1/10 degree; removed, history in DESIGN.md 4.)
//   K2 halos       : compact pass over halo cells only (x-halo columns, north fold rows, zero
//                    south rows of the coordinates, row-Ny substitution of the y-Center metrics).
//                    Round 6 built and measured the alternative (the tile kernel pushes these cells itself, K0 + K1 is the
//                    whole build): nothing gained against the round-5 binary, not adopted, and the code has since been removed.
//                    The record: DESIGN.md 6, profiles/r06/build_push_ab*.txt, profiles/halo_push_removed/.
//   K3 south       : lat-lon continuation rows j = 1-Hy..1 of the 12 metrics (south rank only).
//
// No inter-rank communication: seam halo rows are the neighbour's interior rows of the same
// analytic function.
#include "tpg_common.hpp"
#include "tpg_math.hpp"
#include "tpg_batch.hpp"
#include "tpg_tiles.hpp"

using namespace tpgm;

// Instruments of the tile kernel, scratch builds only (make GRID_FLAGS=-DTPG_CELLS_PROBE=n), never built into a library that a test or the
// bench loads.  profiles/cells_floor: 1 store-only, 2 compute-only (values folded, one store per lane), 3 = 2 without the table loads;
// results are WRONG by design.  profiles/cells_prologue: 4 = the prologue's load order of today with the index arithmetic of before (the
// divisions by tiles_x, the per-lane test of wrap_col, sign-extended 64-bit table addresses); results are right.
#ifndef TPG_CELLS_PROBE
#define TPG_CELLS_PROBE 0
#endif

namespace {

constexpr double kC180Pi = 180.0 / kPi;
constexpr double kC360Pi = 360.0 / kPi;

struct GridK {
    int Nx, Ny, Hx, Hy;
    int shift;            // Nx / 4
    int jstart, jend;     // owned global rows
    int jm_lo, jm_hi;     // global rows whose interior cells this rank evaluates
    int sx, rows;         // local padded extents
    int ft;
    double fplp90;        // first_pole_longitude + 90
    double R;
    // workspace tables
    const double* ti;     // [4][Nx]: a*sind(lf), a*cosd(lf), a*sind(lc), a*cosd(lc), post-shift index
    const double* tj;     // [4][Ny]: sinh/cosh(psi) at Face rows, then at Center rows
    const double* ts;     // [5][Hy+1]: dx_c, dx_f, az_c, az_f, dy for j = 1-Hy..1
};

struct OutPtrs { void* p[TPG_NUM_ARRAYS]; };

struct TableArgs {
    int Nx, Ny, Hy, shift, ft;
    double south, npl, R;
    double* ti; double* tj; double* ts;
};

// ---- 1-D tables (src/tripolar_grid.jl:76-97) ------------------------------------------------
__device__ double lambda_face(int i, int N, int ft)
{
    long long num = 360ll * (i - 1) - 180ll * N;
    if (ft == TPG_F32) return (double)((float)num / (float)N);
    return (double)num / (double)N;
}
__device__ double lambda_center(int i, int N, int ft)
{
    long long num = 360ll * (2ll * i - 1) - 360ll * N;
    if (ft == TPG_F32) return (double)((float)num / (float)(2ll * N));
    return (double)num / (double)(2ll * N);
}
__device__ double phi_center(int j, int N, double south)
{
    if (N == 1) return south;
    if (south == __builtin_rint(south) && absD(south) < 1e6) {
        long long s = (long long)south;
        long long num = s * (N - 1) + (90 - s) * (long long)(j - 1);
        return (double)num / (double)(N - 1);
    }
    dd step = dd_div(two_sum(90.0, -south), dd{ (double)(N - 1), 0.0 });
    dd v = dd_add(dd{ south, 0.0 }, dd_mul_d(step, (double)(j - 1)));
    return v.hi + v.lo;
}

__global__ __launch_bounds__(64) void k_tables(TableArgs t)
{
    int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const double a = tand((90.0 - t.npl) / 2);               // focal_distance, :76
    if (tid < t.Nx) {
        int is = tid + 1;
        int i0 = is - t.shift; if (i0 < 1) i0 += t.Nx;        // circshift folded into the index (:121-130)
        double lf = lambda_face(i0, t.Nx, t.ft), lc = lambda_center(i0, t.Nx, t.ft);
        double slf = sind(lf), clf = cosd(lf), slc = sind(lc), clc = cosd(lc);
        if (t.ft == TPG_F32) {   // sind(::Float32) returns Float32 in the reference
            slf = (double)(float)slf; clf = (double)(float)clf; slc = (double)(float)slc; clc = (double)(float)clc;
        }
        t.ti[0 * t.Nx + tid] = a * slf;
        t.ti[1 * t.Nx + tid] = a * clf;
        t.ti[2 * t.Nx + tid] = a * slc;
        t.ti[3 * t.Nx + tid] = a * clc;
        return;
    }
    tid -= t.Nx;
    if (tid < 2 * t.Ny) {
        int face = tid < t.Ny;
        int j = (face ? tid : tid - t.Ny) + 1;
        double pc = phi_center(j, t.Ny, t.south);
        double phi = pc;
        if (face) {
            double dphi = t.Ny > 1 ? phi_center(2, t.Ny, t.south) - phi_center(1, t.Ny, t.south) : 0.0;   // :96
            phi = pc - dphi / 2;                                                                          // :97
        }
        double psi = asinhD(tand((90.0 - phi) / 2) / a);      // generate_tripolar_coordinates.jl:66
        double sh, ch;
        sinh_cosh(psi, sh, ch);
        int base = face ? 0 : 2;
        t.tj[(base + 0) * t.Ny + (j - 1)] = sh;
        t.tj[(base + 1) * t.Ny + (j - 1)] = ch;
        return;
    }
    tid -= 2 * t.Ny;
    if (tid <= t.Hy) {
        // lat-lon continuation rows (src/tripolar_grid.jl:277-300); Oceananigans
        // LatitudeLongitudeGrid metric formulas, SURVEY.md Appendix A-8
        int j = 1 - t.Hy + tid;
        const double south = t.south, R = t.R;
        const double dlam = 360.0 / (double)t.Nx;
        const double dphiL = (90.0 - south) / (double)t.Ny;
        double pf, pfn, pc, pcm;
        if (south == __builtin_rint(south)) {
            long long s = (long long)south, Ny = t.Ny;
            pf  = (double)(s * Ny + (90 - s) * (long long)(j - 1)) / (double)Ny;
            pfn = (double)(s * Ny + (90 - s) * (long long)j) / (double)Ny;
            pc  = (double)(2 * s * Ny + (90 - s) * (long long)(2 * j - 1)) / (double)(2 * Ny);
            pcm = (double)(2 * s * Ny + (90 - s) * (long long)(2 * j - 3)) / (double)(2 * Ny);
        } else {
            pf  = south + (double)(j - 1) * dphiL;
            pfn = south + (double)j * dphiL;
            pc  = south + ((double)(2 * j - 1) * (90.0 - south)) / (double)(2 * t.Ny);
            pcm = south + ((double)(2 * j - 3) * (90.0 - south)) / (double)(2 * t.Ny);
        }
        int n = t.Hy + 1;
        t.ts[0 * n + tid] = R * (dlam * kDeg2Rad) * cosD(kPi * pc / 180);
        t.ts[1 * n + tid] = R * (dlam * kDeg2Rad) * cosD(kPi * pf / 180);
        t.ts[2 * n + tid] = R * R * (dlam * kDeg2Rad) * (sinD(kPi * pfn / 180) - sinD(kPi * pf / 180));
        t.ts[3 * n + tid] = R * R * (dlam * kDeg2Rad) * (sinD(kPi * pc / 180) - sinD(kPi * pcm / 180));
        t.ts[4 * n + tid] = R * (dphiL * kDeg2Rad);
    }
}

// ---- the Murray (1996) map at one staggered point (generate_tripolar_coordinates.jl:66-87) ----
struct LP { double lam, phi; };

__device__ __forceinline__ LP analytic(const GridK& g, int xl, int yl, int is, int js)
{
    int i0 = is - g.shift; if (i0 < 1) i0 += g.Nx;           // pre-shift index drives the :75/:82 branches
    const double* ti = g.ti + (xl == TPG_FACE ? 0 : 2) * g.Nx;
    const double* tj = g.tj + (yl == TPG_FACE ? 0 : 2) * g.Ny;
    double asl = ti[is - 1], acl = ti[g.Nx + is - 1];
    double sh = tj[js - 1], ch = tj[g.Ny + js - 1];
    double x = asl * ch;                                     // :67
    double y = acl * sh;                                     // :68
    bool pole = (x == 0.0) & (y == 0.0);                     // :74
    double l = pole ? (i0 == 1 ? -90.0 : 90.0) : -kC180Pi * atanD(y / x);   // :75-77
    LP r;
    r.phi = 90.0 - kC360Pi * atanD(sqrt(y * y + x * x));     // :78
    l += (i0 <= g.Nx / 2) ? -90.0 : 90.0;                    // :82
    l += g.fplp90;                                           // :86
    r.lam = fmod360(fmod360(l) + 360.0);                     // :87, OrthogonalSphericalShellGrids.jl:24
    return r;
}

// x index of the fold partner (zipper_boundary_condition.jl:73-75, :90-92, :110, :125)
__device__ __forceinline__ int fold_partner(int xl, int i, int Nx)
{
    int ip = (xl == TPG_FACE) ? Nx - i + 2 : Nx - i + 1;
    return ip > Nx ? ip - Nx : ip;
}

// Value of the halo-filled coordinate field of location (xl,yl) at logical (i,j), i in 0..Nx+1,
// j in 0..Ny+1: the composition of periodic x, north fold (sign +1, src/tripolar_grid.jl:147),
// row-Ny substitution (zipper_boundary_condition.jl:102,135) and the zero south halo (:148).
__device__ __forceinline__ LP coord(const GridK& g, int xl, int yl, int i, int j)
{
    if (j < 1) return LP{ 0.0, 0.0 };
    int iw = i < 1 ? i + g.Nx : (i > g.Nx ? i - g.Nx : i);
    int js = j;
    if (j > g.Ny) {
        int dj = j - g.Ny;
        js = (yl == TPG_FACE) ? g.Ny - dj + 1 : g.Ny - dj;
        iw = fold_partner(xl, iw, g.Nx);
        if (js < 1) return LP{ 0.0, 0.0 };
    } else if (j == g.Ny && yl == TPG_CENTER && iw > g.Nx / 2) {
        iw = fold_partner(xl, iw, g.Nx);
    }
    return analytic(g, xl, yl, iw, js);
}

// Distances.haversine((l1,p1),(l2,p2),R), call sites src/tripolar_grid_utils.jl:13-21
__device__ __forceinline__ double haversine(LP a, LP b, double R)
{
    double dl = (b.lam - a.lam) * kDeg2Rad;
    double a1 = a.phi * kDeg2Rad;
    double a2 = b.phi * kDeg2Rad;
    double dp = a2 - a1;
    double s1 = sinD(dp / 2), s2 = sinD(dl / 2);
    double h = s1 * s1 + cosD(a1) * cosD(a2) * (s2 * s2);
    double r = sqrt(h);
    return 2 * (R * asinD(r != r ? r : (r < 1.0 ? r : 1.0)));
}

struct V3 { double x, y, z; };
// Oceananigans lat_lon_to_cartesian(phi, lambda, 1)
__device__ __forceinline__ V3 cartesian(LP p)
{
    double cl = cosd(p.phi);
    return V3{ cosd(p.lam) * cl, sind(p.lam) * cl, sind(p.phi) };
}
__device__ __forceinline__ double dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b)
{
    return V3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x };
}
// Oceananigans spherical_area_triangle / spherical_area_quadrilateral
__device__ __forceinline__ double tri_area(V3 a, V3 b, V3 c)
{
    double t = absD(dot3(a, cross3(b, c)));
    t /= 1 + dot3(a, b) + dot3(b, c) + dot3(a, c);
    return 2 * atanD(t);
}
__device__ __forceinline__ double quad_area(V3 a, V3 b, V3 c, V3 d)
{
    double A = tri_area(a, b, c);
    A += tri_area(a, b, d);
    A += tri_area(a, c, d);
    A += tri_area(b, c, d);
    return A / 2;
}

// tan(E/2) of one spherical triangle through the unscaled division (tpgm::div_nr).  The denominator
// 1 + a.b + b.c + a.c of unit vectors is 0 or at least ~1e-16 in magnitude and at most 4; a zero gives
// NaN here (rcp(0) = inf), which the callers' atan_small_b reports as `rare`, and their fallback
// recomputes the four tangents with IEEE `/` (tri_tan).
__device__ __forceinline__ double tri_num(V3 a, V3 b, V3 c) { return absD(dot3(a, cross3(b, c))); }
__device__ __forceinline__ double tri_den(V3 a, V3 b, V3 c) { return 1 + dot3(a, b) + dot3(b, c) + dot3(a, c); }
__device__ __forceinline__ double tri_tan_nr(V3 a, V3 b, V3 c) { return div_nr(tri_num(a, b, c), tri_den(a, b, c)); }
__device__ __forceinline__ double tri_tan(V3 a, V3 b, V3 c)
{
    return absD(dot3(a, cross3(b, c))) / (1 + dot3(a, b) + dot3(b, c) + dot3(a, c));
}

// NT = streaming store: the 20 output arrays (1 GB at 1/10 deg) are written once and not re-read by
// this launch sequence; a plain store would park them as dirty lines in L2 / Infinity Cache and
// the NEXT kernel on the stream (typically a halo fill) would pay for their eviction.
template <typename T, bool NT = false>
__device__ __forceinline__ void put(const OutPtrs& o, int q, long long off, double v)
{
    T* p = static_cast<T*>(o.p[q]) + off;
    if (NT) __builtin_nontemporal_store((T)v, p); else *p = (T)v;
}

// The tile kernel addresses its stores as (uniform base pointer) + (32-bit BYTE offset in a VGPR): the saddr form of
// global_store takes exactly that, so the 20 stores of a cell share two offset registers instead of each paying a 64-bit
// v_lshl_add_u64 for its own address (round 3).  Valid while one array is smaller than 4 GiB -- the launcher checks.
template <typename T, bool NT = false, bool PIN = true>
__device__ __forceinline__ void put32(const OutPtrs& o, int q, unsigned boff, double v)
{
    // the empty asm keeps the zero-extension of the offset next to its store: hoisted and shared as a 64-bit pair, it would no
    // longer match the saddr addressing pattern and every store would pay a 64-bit add again
    if (PIN) asm volatile("" : "+v"(boff));
    T* p = reinterpret_cast<T*>(static_cast<char*>(o.p[q]) + boff);
    if (NT) __builtin_nontemporal_store((T)v, p); else *p = (T)v;
}
// The asm of put32 costs a v_mov_b32 per store whose offset is used again afterwards (the operand is read-write, so the compiler copies
// it first).  A run of stores in ONE basic block needs one pinned copy only: the zero-extension cannot leave the block without passing
// the asm, and inside the block every store still selects base + zext(offset).  pin_off + put32<T, NT, false> is that form.
__device__ __forceinline__ unsigned pin_off(unsigned boff)
{
    asm volatile("" : "+v"(boff));
    return boff;
}

// ---- K1: interior cells ------------------------------------------------------------------------
template <typename T, bool NT>
__global__ __launch_bounds__(256) void k_cells(GridK g, OutPtrs o)
{
    const int nbx = (g.Nx + 255) / 256;
    int rb = blockIdx.x / nbx;
    int i = (blockIdx.x - rb * nbx) * 256 + threadIdx.x + 1;
    int j = g.jm_lo + rb;
    if (i > g.Nx) return;

    LP cc = coord(g, 0, 0, i, j), fc = coord(g, 1, 0, i, j), cf = coord(g, 0, 1, i, j), ff = coord(g, 1, 1, i, j);
    LP fc_e = coord(g, 1, 0, i + 1, j), fc_s = coord(g, 1, 0, i, j - 1);
    LP cc_w = coord(g, 0, 0, i - 1, j), cc_s = coord(g, 0, 0, i, j - 1), cc_sw = coord(g, 0, 0, i - 1, j - 1);
    LP ff_e = coord(g, 1, 1, i + 1, j), ff_n = coord(g, 1, 1, i, j + 1), ff_ne = coord(g, 1, 1, i + 1, j + 1);
    LP cf_w = coord(g, 0, 1, i - 1, j), cf_n = coord(g, 0, 1, i, j + 1);

    const double R = g.R;
    double dxcc = haversine(fc_e, fc, R);      // tripolar_grid_utils.jl:13
    double dxfc = haversine(cc, cc_w, R);      // :14
    double dxcf = haversine(ff_e, ff, R);      // :15
    double dxff = haversine(cf, cf_w, R);      // :16
    double dycc = haversine(cf_n, cf, R);      // :18
    double dyfc = haversine(ff_n, ff, R);      // :19
    double dycf = haversine(cc, cc_s, R);      // :20
    double dyff = haversine(fc, fc_s, R);      // :21
    double azcc = quad_area(cartesian(ff), cartesian(ff_e), cartesian(ff_ne), cartesian(ff_n)) * (R * R);   // :23-28
    double azfc = dyfc * dxfc;                 // :34
    double azcf = dycf * dxcf;                 // :35
    double azff = quad_area(cartesian(cc_sw), cartesian(cc_s), cartesian(cc), cartesian(cc_w)) * (R * R);   // :38-43

    long long off = (long long)(i + g.Hx - 1) + (long long)g.sx * (j - g.jstart + g.Hy);
    put<T, NT>(o, TPG_LAMBDA_CC, off, cc.lam); put<T, NT>(o, TPG_LAMBDA_FC, off, fc.lam);
    put<T, NT>(o, TPG_LAMBDA_CF, off, cf.lam); put<T, NT>(o, TPG_LAMBDA_FF, off, ff.lam);
    put<T, NT>(o, TPG_PHI_CC, off, cc.phi); put<T, NT>(o, TPG_PHI_FC, off, fc.phi);
    put<T, NT>(o, TPG_PHI_CF, off, cf.phi); put<T, NT>(o, TPG_PHI_FF, off, ff.phi);
    put<T, NT>(o, TPG_DX_CC, off, dxcc); put<T, NT>(o, TPG_DX_FC, off, dxfc);
    put<T, NT>(o, TPG_DX_CF, off, dxcf); put<T, NT>(o, TPG_DX_FF, off, dxff);
    put<T, NT>(o, TPG_DY_CC, off, dycc); put<T, NT>(o, TPG_DY_CF, off, dycf);
    put<T, NT>(o, TPG_DY_FC, off, dyfc); put<T, NT>(o, TPG_DY_FF, off, dyff);
    put<T, NT>(o, TPG_AZ_CC, off, azcc); put<T, NT>(o, TPG_AZ_FC, off, azfc);
    put<T, NT>(o, TPG_AZ_CF, off, azcf); put<T, NT>(o, TPG_AZ_FF, off, azff);
}

// ---- shared point records of the work-sharing form (k_cells_tile) ------------------------------------
// Every staggered point (lambda, phi) and what the metrics derive from it -- a = deg2rad(phi),
// cos(a) for the haversines, the unit vector for the two quadrilateral areas -- is evaluated ONCE
// by the thread that owns it and shared with the cells around it: ~65 instead of ~140 transcendental
// calls per cell.  The arithmetic of every value is unchanged (same operation sequence), so results
// are bit-identical to k_cells.
struct Pt  { double lam, phi, a, ca; };                 // FC / CF points
struct PtX { double lam, phi, a, ca, X, Y, Z; };        // CC / FF points (+ unit vector)
struct Nb  { double lam, a, ca; };                      // what a haversine needs of a neighbour
struct NbX { double lam, a, ca, X, Y, Z; };

__device__ __forceinline__ Pt make_pt(const GridK& g, int xl, int yl, int i, int j)
{
    LP p = coord(g, xl, yl, i, j);
    Pt r; r.lam = p.lam; r.phi = p.phi; r.a = p.phi * kDeg2Rad; r.ca = cosD(r.a);
    return r;
}
__device__ __forceinline__ PtX make_ptx(const GridK& g, int xl, int yl, int i, int j)
{
    LP p = coord(g, xl, yl, i, j);
    PtX r; r.lam = p.lam; r.phi = p.phi; r.a = p.phi * kDeg2Rad; r.ca = cosD(r.a);
    double sl, cl, sp, cp;
    sincosd(p.lam, sl, cl);
    sincosd(p.phi, sp, cp);
    r.X = cl * cp; r.Y = sl * cp; r.Z = sp;             // lat_lon_to_cartesian(phi, lambda, 1)
    return r;
}
__device__ __forceinline__ Nb nb_of(const Pt& p) { return Nb{ p.lam, p.a, p.ca }; }
__device__ __forceinline__ Nb nb_of(const PtX& p) { return Nb{ p.lam, p.a, p.ca }; }
__device__ __forceinline__ NbX nbx_of(const PtX& p) { return NbX{ p.lam, p.a, p.ca, p.X, p.Y, p.Z }; }
__device__ __forceinline__ V3 v3_of(const PtX& p) { return V3{ p.X, p.Y, p.Z }; }
__device__ __forceinline__ V3 v3_of(const NbX& p) { return V3{ p.X, p.Y, p.Z }; }

template <int DIR> __device__ __forceinline__ double shf(double v)
{
    return DIR > 0 ? __shfl_down(v, 1, 64) : __shfl_up(v, 1, 64);   // DIR>0: value of lane+1
}
template <int DIR> __device__ __forceinline__ Nb shf_nb(const Pt& p)
{
    return Nb{ shf<DIR>(p.lam), shf<DIR>(p.a), shf<DIR>(p.ca) };
}
template <int DIR> __device__ __forceinline__ NbX shf_nbx(const PtX& p)
{
    return NbX{ shf<DIR>(p.lam), shf<DIR>(p.a), shf<DIR>(p.ca), shf<DIR>(p.X), shf<DIR>(p.Y), shf<DIR>(p.Z) };
}

// haversine(x, y, R) with the per-point parts precomputed: x = first argument, y = second
__device__ __forceinline__ double hav(double xlam, double xa, double xca, double ylam, double ya, double yca, double R)
{
    double dl = (ylam - xlam) * kDeg2Rad;
    double dp = ya - xa;
    double s1 = sinD(dp / 2), s2 = sinD(dl / 2);
    double h = s1 * s1 + xca * yca * (s2 * s2);
    double r = sqrt(h);
    return 2 * (R * asinD(r != r ? r : (r < 1.0 ? r : 1.0)));
}
#define HAV(P, Q) hav((P).lam, (P).a, (P).ca, (Q).lam, (Q).a, (Q).ca, R)


// ---- one point set = the 4 points a tile thread creates, on the straight-line batch forms ----------
//  * rows j < Ny need no fold / substitution / pole logic, so a lane's lambda-table values
//    (a sind, a cosd at its Face and Center column) and the per-row psi-table values (wave-uniform)
//    feed the Murray map directly; the index maps of coord() are left to the special rows;
//  * all transcendentals are evaluated by the straight-line batch forms of tpg_batch.hpp
//    (independent chains per basic block), with rare cases patched afterwards.
struct Step4 {           // the 4 points a step creates: k = 0 FC(jc), 1 CC(jc), 2 FF(jf), 3 CF(jf)
    double lam[4], phi[4], a[4], ca[4];
    double X[2], Y[2], Z[2];     // 0: CC, 1: FF
};

struct LaneConst { double aslF, aclF, aslC, aclC, hemi; };

struct RowTab { double shC, chC, shF, chF; };    // sinh/cosh(psi) of Center row jc and Face row jf: wave-uniform

// Scalar (s_load) read of the psi tables: the row index is wave-uniform and the tables were written by
// the previous kernel, so they can be read through the constant address space into SGPRs -- no VGPRs,
// and issued one row ahead so the latency never sits on the critical path.
// The four entries are addressed as (table base) + (32-bit unsigned BYTE offset): the clamped rows are >= 1, so no index is negative and
// none needs the sign-extended 64-bit address arithmetic that int indices cost (Ny < 2^27: the launcher checks).
typedef const double __attribute__((address_space(4))) kconst_double;
typedef const char __attribute__((address_space(4))) kconst_char;
__device__ __forceinline__ RowTab load_rowtab(const GridK& g, int jc, int jf)
{
    jc = __builtin_amdgcn_readfirstlane(jc < 1 ? 1 : (jc > g.Ny ? g.Ny : jc));
    jf = __builtin_amdgcn_readfirstlane(jf < 1 ? 1 : (jf > g.Ny ? g.Ny : jf));
#if TPG_CELLS_PROBE == 4
    kconst_double* tj = (kconst_double*)g.tj;
    return RowTab{ tj[2 * g.Ny + jc - 1], tj[3 * g.Ny + jc - 1], tj[0 * g.Ny + jf - 1], tj[1 * g.Ny + jf - 1] };
#else
    kconst_char* tj = (kconst_char*)g.tj;
    const unsigned ny8 = 8u * (unsigned)g.Ny, c8 = 8u * (unsigned)(jc - 1), f8 = 8u * (unsigned)(jf - 1);
    auto at = [&](unsigned boff) -> double { return *(kconst_double*)(tj + boff); };
    return RowTab{ at(2u * ny8 + c8), at(3u * ny8 + c8), at(f8), at(ny8 + f8) };
#endif
}

__device__ __forceinline__ void points_fast(const GridK& g, const LaneConst& lc, const RowTab& rt, Step4& s, const double* atab)
{
    const double shC = rt.shC, chC = rt.chC, shF = rt.shF, chF = rt.chF;
    double x[4] = { lc.aslF * chC, lc.aslC * chC, lc.aslF * chF, lc.aslC * chF };          // :67
    double y[4] = { lc.aclF * shC, lc.aclC * shC, lc.aclF * shF, lc.aclC * shF };          // :68
    double q[4], rr[4], at1[4], at2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { q[k] = y[k] / x[k]; rr[k] = sqrt_nr<true>(y[k] * y[k] + x[k] * x[k]);   /* > 0: no pole below row Ny */ }
    tpgb::atan_tab_b<4>(q, at1, atab);
    tpgb::atan_tab_b<4, true>(rr, at2, atab);      // rr = sqrt(...) of finite table products
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double l = -kC180Pi * at1[k];                          // :77 (no pole below row Ny)
        s.phi[k] = 90.0 - kC360Pi * at2[k];                    // :78
        l += lc.hemi;                                          // :82
        l += g.fplp90;                                         // :86
        s.lam[k] = tpgb::fmod360_pos(tpgb::fmod360_small(l) + 360.0);     // :87
        s.a[k] = s.phi[k] * kDeg2Rad;
    }
    if (tpgb::cos_b<4>(s.a, s.ca)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s.ca[k] = cosD(s.a[k]);
    }
    double ang[4] = { s.lam[1], s.phi[1], s.lam[2], s.phi[2] }, sn[4], cs[4];
    tpgb::sincosd_b<4>(ang, sn, cs);
    s.X[0] = cs[0] * cs[1]; s.Y[0] = sn[0] * cs[1]; s.Z[0] = sn[1];      // CC
    s.X[1] = cs[2] * cs[3]; s.Y[1] = sn[2] * cs[3]; s.Z[1] = sn[3];      // FF
}

// ---- the tile kernel's point set (the arithmetic of points_fast in batches of 2: 4 waves/SIMD, under 128 VGPRs): each chain of a lambda -> -lambda column pair is evaluated once ------------------------
// A point's chain -- y / x, sqrt(y^2 + x^2), the two table atans, phi, cos(deg2rad phi) and, for CC / FF, sind / cosd(phi) --
// depends on its column only through |a sind(lambda)| and |a cosd(lambda)|.  The lambda tables are num / N with an integer num,
// and the column i' = 2 shift + 2 - i (Face), 2 shift + 1 - i (Center), mod Nx, has exactly -num: sind negates exactly, cosd is
// unchanged, x' = -x, y' = y, and every later operation of the chain is sign-symmetric.  So |atan(y / x)|, phi, cos and the
// latitude sine / cosine of the two columns are the same bits (tests/test_pair_premise.py; DESIGN.md 4 records why the fold
// partner and i + Nx/2 must NOT be used: lambda +- 180 is not representable at Nx = 3600).
// A wave holds two half-wave strips that are such images of each other (see k_cells_tile).  Lanes 0-31 evaluate the two Center-x
// chains CC(jc), CF(jf) of their column and sind / cosd of CC's latitude, lanes 32-63 the two Face-x chains FC(jc), FF(jf) and
// sind / cosd of FF's latitude; the code is the same, the half only selects the table entries.  Each lane parks its 8 doubles in
// the wave's own rows of the tile's LDS (they hold the point records only later), row = 3 k + {at1, phi, ca} of point k and
// 12.. = sind / cosd(phi) of CC, FF, and every lane reads the rows of all four points back: its own two from its own slot, the
// other two from lane 63 - l (Center) or 64 - l (Face), the lane that holds the image column.  The exchange therefore is the
// permutation into the slots k as well: no select and no cross-lane VALU.  LDS operations of one wave execute in order; the
// wave-scope fences keep the compiler from moving accesses across the exchange.
// Sign of at1: atan(y / x) carries sign(y) xor sign(x), for every finite pair (the zero-x patch to +-pi/2 included, which stays
// with the owner).  The two Face columns lambda = -180 and 0 are their own images, x = -+0 there, so the receiver must not negate
// blindly: every lane gives |at1| the sign of ITS OWN y / x.  The sign of a product is the xor of its factors' signs, cosh > 0
// and sinh(psi) is wave-uniform, so that sign is sign(a sind) xor sign(a cosd) xor sign(sinh): integer work on the high words.
// (Applied to a lane's own chains too, where it is the identity except on a zero at1, whose sign the next operation,
// -180/pi at1 + (+-90), drops.)  a = deg2rad(phi) is recomputed by every lane.  Everything after the chain is points_fast's, per lane.
template <int R>
__device__ __forceinline__ void points_pair(const GridK& g, const LaneConst& lc, const RowTab& rt, Step4& s, const double* atab,
                                            double (*L)[R][64], int p, int lane)
{
    const bool face = lane >= 32;
    const double aslO = face ? lc.aslF : lc.aslC, aclO = face ? lc.aclF : lc.aclC;      // the x-location this lane evaluates
    {
        const double x[2] = { aslO * rt.chC, aslO * rt.chF };                               // :67  own chain 0: row jc, 1: row jf
        const double y[2] = { aclO * rt.shC, aclO * rt.shF };                               // :68
        double q[2], rr[2], at1[2], at2[2], phi[2], a[2], ca[2];
        // y / x through the unscaled division: both are products of finite table entries of moderate size (|x| is 0 on the two pole
        // meridians, else >= ~1e-17; tests/test_gpu_math.py checks div_nr against IEEE on that range).  A zero denominator is the one case
        // that needs IEEE semantics (y / +-0 = +-Inf, and atan(+-Inf) = +-pi/2): those lanes are patched after the table atan, which can
        // then take the FINITE form for every lane (no clamp of the argument; a NaN from div_nr(y, 0) just flows through the discarded lane).
        bool zerox = false;
#pragma unroll
        for (int m = 0; m < 2; ++m) { q[m] = div_nr(y[m], x[m]); zerox |= TPG_RARE(x[m] == 0.0); rr[m] = sqrt_nr<true>(y[m] * y[m] + x[m] * x[m]);   /* > 0: no pole below row Ny */ }
        // the ABS form, no copysign: only |at1| is used (its sign is rebuilt after the exchange, below), and rr > 0
        tpgb::atan_tab_b<2, true, true>(q, at1, atab);
        tpgb::atan_tab_b<2, true, true>(rr, at2, atab);
        if (zerox) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
                if (x[m] == 0.0) {
                    // msun: atan(+-Inf) = +-(atanhi[3] + atanlo[3]) = +-pi/2 (the table row gives hi - ((-0 - lo) - t) = RN(hi + lo) = hi as well);
                    // 0 / 0 stays NaN
                    const double qq = y[m] / x[m];
                    at1[m] = (qq != qq) ? qq : csign(kPio2Hi, qq);
                }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) { phi[m] = 90.0 - kC360Pi * at2[m]; a[m] = phi[m] * kDeg2Rad; }     // :78
        if (tpgb::cos_lat_b<2>(a, ca)) { ca[0] = cosD(a[0]); ca[1] = cosD(a[1]); }
        double lat[1] = { face ? phi[1] : phi[0] }, sp[1], cp[1];                          // FF(jf) | CC(jc)
        if (tpgb::sincosd_lat_b<1>(lat, sp, cp)) tpgb::sincosd_b<1>(lat, sp, cp);
        const int k0 = face ? 0 : 1;                                                       // point of chain 0; chain 1 is point k0 + 2
        L[3 * k0 + 0][p][lane] = at1[0]; L[3 * k0 + 1][p][lane] = phi[0]; L[3 * k0 + 2][p][lane] = ca[0];
        L[3 * k0 + 6][p][lane] = at1[1]; L[3 * k0 + 7][p][lane] = phi[1]; L[3 * k0 + 8][p][lane] = ca[1];
        L[14 - 2 * k0][p][lane] = sp[0]; L[15 - 2 * k0][p][lane] = cp[0];                  // 12, 13: CC; 14, 15: FF
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // lane 0 has no Face image (64 - 0); it is a west apron, whose Face points nobody reads: any finite chain will do
    const int srcF = face ? lane : (lane == 0 ? 63 : 64 - lane), srcC = face ? 63 - lane : lane;
    // the sign of at1 as a word with bit 31 only: the lane's part (one per x-location) and the row's part (wave-uniform, scalar).  It is
    // applied around the product -180/pi |at1| below -- (-c) (s |t|) = s ((-c) |t|) bit for bit, a product's sign is the xor of its
    // factors' -- where |at1| is an operand modifier, the row's part rides on the constant and the lane's part is one xor per point
    const int sgn = (int)0x80000000;
    int sgJc = __double2hiint(rt.shC) & sgn, sgJf = __double2hiint(rt.shF) & sgn;
    int sgF = (__double2hiint(lc.aslF) ^ __double2hiint(lc.aclF)) & sgn, sgC = (__double2hiint(lc.aslC) ^ __double2hiint(lc.aclC)) & sgn;
    asm volatile("" : "+v"(sgF), "+v"(sgC), "+s"(sgJc), "+s"(sgJf));     // keeps the parts masked: re-associated to (a ^ b) & m, every point pays the mask again
    double at1[4], sp[2], cp[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int src = (k == 0 || k == 2) ? srcF : srcC;
        at1[k] = L[3 * k + 0][p][src];
        s.phi[k] = L[3 * k + 1][p][src];
        s.ca[k] = L[3 * k + 2][p][src];
    }
    sp[0] = L[12][p][srcC]; cp[0] = L[13][p][srcC];
    sp[1] = L[14][p][srcF]; cp[1] = L[15][p][srcF];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                                                       // the records go into these rows next
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // |-180/pi at1 + (+-90)| <= 180 + 2 ulp, so with |fplp90| < 179 (wave-uniform; the default pole longitude gives 160) |l| < 360 and the
    // first fmod is the identity: csign(|l| - 0, l) = l
    const bool lsmall = (__double2hiint(g.fplp90) & 0x7fffffff) < 0x40666000;     // |fplp90| < 179 on the high word: a scalar compare
    const double cJc = __hiloint2double(__double2hiint(-kC180Pi) ^ sgJc, __double2loint(-kC180Pi));      // -180/pi with the row's sign: scalar
    const double cJf = __hiloint2double(__double2hiint(-kC180Pi) ^ sgJf, __double2loint(-kC180Pi));
    double l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double m = ((k < 2) ? cJc : cJf) * absD(at1[k]);  // :77 (no pole below row Ny)
        l[k] = __hiloint2double(__double2hiint(m) ^ ((k == 0 || k == 2) ? sgF : sgC), __double2loint(m));
        l[k] += lc.hemi;                                       // :82
        l[k] += g.fplp90;                                      // :86
        s.a[k] = s.phi[k] * kDeg2Rad;
    }
    if (lsmall) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s.lam[k] = tpgb::fmod360_pos(l[k] + 360.0);                            // :87
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) s.lam[k] = tpgb::fmod360_pos(tpgb::fmod360_small(l[k]) + 360.0);       // :87
    }
    double lon[2] = { s.lam[1], s.lam[2] }, sl[2], cl[2];
    tpgb::sincosd_b<2, true>(lon, sl, cl);                               // POS: lam = fmod360_pos(y + 360), |y| < 360, lies in [+0, 360] -- sign bit clear
    s.X[0] = cl[0] * cp[0]; s.Y[0] = sl[0] * cp[0]; s.Z[0] = sp[0];      // CC
    s.X[1] = cl[1] * cp[1]; s.Y[1] = sl[1] * cp[1]; s.Z[1] = sp[1];      // FF
}

// stored column of a strip lane, wrapped into 1..Nx: tpgt::wrap_col (tpg_tiles.hpp).  This is the form of before, whose test for the
// generic modulo is per lane; only the probe TPG_CELLS_PROBE = 4 still uses it.
__device__ __forceinline__ int wrap_col_per_lane(int v, int Nx)
{
    if (v < 1) v += Nx;
    if (v > Nx) v -= Nx;
    if (v < 1 || v > Nx) { v = (v - 1) % Nx; v = (v < 0 ? v + Nx : v) + 1; }
    return v;
}

// general rows (row Ny: fold, substitution, pole; any row when |fplp90| > 360) through coord()
__device__ __noinline__ void points_general(const GridK& g, int i, int jc, int jf, Step4& s)
{
    Pt fc = make_pt(g, 1, 0, i, jc), cf = make_pt(g, 0, 1, i, jf);
    PtX cc = make_ptx(g, 0, 0, i, jc), ff = make_ptx(g, 1, 1, i, jf);
    s.lam[0] = fc.lam; s.phi[0] = fc.phi; s.a[0] = fc.a; s.ca[0] = fc.ca;
    s.lam[1] = cc.lam; s.phi[1] = cc.phi; s.a[1] = cc.a; s.ca[1] = cc.ca;
    s.lam[2] = ff.lam; s.phi[2] = ff.phi; s.a[2] = ff.a; s.ca[2] = ff.ca;
    s.lam[3] = cf.lam; s.phi[3] = cf.phi; s.a[3] = cf.a; s.ca[3] = cf.ca;
    s.X[0] = cc.X; s.Y[0] = cc.Y; s.Z[0] = cc.Z;
    s.X[1] = ff.X; s.Y[1] = ff.Y; s.Z[1] = ff.Z;
}

// ---- K1 (tile form): 64 x R point sets per block through LDS, 4 waves per SIMD -------------------
// Sharing points through registers (a wave marching north with the previous row live) needs ~70 live doubles
// per lane: 2 waves/SIMD, where dependent FP64 chains leave the VALU idle ~28 % of the time (PMC, round 1); the
// plain thread-per-cell kernel at 4 waves/SIMD is 95 % busy.  This form keeps the work-sharing but not the
// register state: a block of 64 x R threads evaluates one point set per thread (step s = FC(s), CC(s),
// FF(s+1), CF(s+1)), parks {lambda, a, cos a[, X, Y, Z]} in LDS
// (18 doubles x 64 x R), and after ONE barrier every thread with a south and east/west neighbour
// inside the tile computes its cell from its own registers plus 48 LDS reads.  Row p = 0 is an apron (tiles
// overlap by one point row); the apron wave, which has no cell row, spends phase 2 on one of the eight haversines
// (Dy_ff) of all rows.
// Columns: a wave holds TWO strips of 32 lanes.  With f1 = shift + 1 the stored column of lambda = -180, lanes 0-31 of
// tile t hold the ascending columns f1 + 30 t - 1 + lane and lane 32 + k holds 2 shift + 1 - (column of lane 31 - k),
// the x-Center lambda -> -lambda image, ascending as well; all wrapped into 1..Nx.  Lanes 0 / 32 are west aprons,
// 31 / 63 east aprons, lanes 1-30 and 33-62 emit: (R-1)/R x 60/64 of the lanes.  The cells f1 .. f1 + Nx/2 - 1 and
// their images partition 1..Nx, so tiles_x = ceil((Nx/2) / 30).  The Center image of lane l's column sits in lane
// 63 - l and the Face image in lane 64 - l: phase 1 evaluates each pair's point chains once (points_pair).
// A wave owns one point row, so the special row Ny and |fplp90| > 360 are a wave-uniform branch to coord(),
// unpaired: every lane evaluates its own column.  (Row 0 used to go there as well; now only its two Center-y points are special.)
// Same arithmetic as k_cells for every value: bit-identical results.
template <int R> struct TileLds { double v[18][R][64]; };
enum { L_FC = 0, L_CC = 3, L_FF = 9, L_CF = 15 };    // field bases: FC(lam,a,ca) CC(lam,a,ca,X,Y,Z) FF(6) CF(3)

// An LDS address in a VGPR that the compiler cannot see through: reads through it keep it as their base register and put everything
// else into the immediate offset (see phase 2 of k_cells_tile).
typedef const double __attribute__((address_space(3))) lds_cdouble;
__device__ __forceinline__ lds_cdouble* lds_base(const double* p)
{
    unsigned a = (unsigned)(uintptr_t)(lds_cdouble*)p;
    asm volatile("" : "+v"(a));
    return (lds_cdouble*)(uintptr_t)a;
}
struct LdsBase { lds_cdouble* p; int plane; };     // the base and the plane of TileLds it points into

// N haversines at once: x = first argument, y = second, each {lambda, deg2rad(phi), cos}; the same
// operation sequence as hav() with the batch forms (rare arguments fall back to the scalar functions)
template <int N>
__device__ __forceinline__ void hav_batch(const Nb (&X)[N], const Nb (&Y)[N], double Rad, double (&d)[N])
{
    double hp[N], hl[N], s1[N], s2[N], hh[N], as[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        // (d lambda * deg2rad) / 2 as ONE product with deg2rad / 2: halving is exact and rounding is scale-invariant (no underflow:
        // a difference of two longitudes is 0 or >= ~1e-14), so RN(x c) / 2 = RN(x (c / 2)) bit for bit
        double dp = Y[e].a - X[e].a;
        hp[e] = dp / 2; hl[e] = (Y[e].lam - X[e].lam) * (kDeg2Rad * 0.5);
    }
    if (tpgb::sin_small_b<N>(hp, s1)) {
#pragma unroll
        for (int e = 0; e < N; ++e) s1[e] = sinD(hp[e]);
    }
    if (tpgb::sin_small_b<N>(hl, s2)) {
#pragma unroll
        for (int e = 0; e < N; ++e) s2[e] = sinD(hl[e]);
    }
#pragma unroll
    for (int e = 0; e < N; ++e) hh[e] = s1[e] * s1[e] + X[e].ca * Y[e].ca * (s2[e] * s2[e]);
    tpgb::asin_sqrt_b<N>(hh, as);                 // asin(min(sqrt(h), 1)): one rare-argument test for the square root, the clamp and the asin
#pragma unroll
    for (int e = 0; e < N; ++e) d[e] = (2 * Rad) * as[e];      // 2 (R asin) = (2 R) asin bit for bit: doubling is exact (2 R: wave-uniform)
}

// ---- tile order ------------------------------------------------------------------------------------------------------------------
// The launch is 1-D: block id -> tile through tile_of_block, tiles counted tx fastest, tile rows NORTH to SOUTH.  Consecutive block ids
// land on different XCDs (id mod 8), so in the plain order the 128-B line that the strips of tiles tx and tx + 1 share is written from
// two different L2s, and a partial-line write costs what a whole line costs.  The store stream, not the arithmetic, sets the kernel's
// floor at sustained clocks (profiles/cells_floor: the kernel with its arithmetic removed takes 97 % of the full kernel's time), so
// the order hands every XCD runs of 8 adjacent tiles: the shared lines meet in one L2.  (The persistent tile loop measured there is
// not in the tree: slower by 8 %.)
// (TPG_CELLS_PROBE: see the top of the file)
#if TPG_CELLS_PROBE == 2 || TPG_CELLS_PROBE == 3
#define TPG_EMIT(A, OFF, V) (fold ^= (unsigned long long)__double_as_longlong(V) + (A), fold_off = (OFF), folded = true)
#define TPG_EMIT_PINNED(A, OFF, V) TPG_EMIT(A, OFF, V)
#else
#define TPG_EMIT(A, OFF, V) put32<T, NT>(o, A, OFF, V)
#define TPG_EMIT_PINNED(A, OFF, V) put32<T, NT, false>(o, A, OFF, V)      // OFF left pin_off() in this basic block
#endif

// The XCD-grouped order itself is tpgt::tile_of_block, and tile -> (tile row, tile column) tpgt::tile_xy (tpg_tiles.hpp).
//
// What the launch fixes comes from the host: tiles_y, and the reciprocal of tiles_x that replaces the wave's divisions (tpgt::divmod_rcp)
struct TileArgs { int tiles_x, tiles, grouped, tiles_y; unsigned tiles_x_rcp; };

// ---- the prologue: two load round trips per wave ---------------------------------------------------------------------------------
// Before its first Float64 instruction a wave needs its kernel arguments, its word of the atan table (one constant image, see
// tpgb::kAtanTable), four lambda-table entries per lane and four psi-table entries per wave.  Only the table entries need something that
// was loaded -- the arguments -- so two round trips suffice: (1) the arguments and the atan word, issued together at the top;
// (2) the table entries, issued as soon as the tile and the column are known.  The atan word goes to LDS only after (2) is in
// flight, and the values of (2) are pinned around that store (empty asm statements), in front of the wave-uniform branch between the
// paired and the general path: left alone, the compiler sinks loads whose only reader is the paired path into that branch, behind every
// wait in front of it.  Nothing in front of the table loads may be a branch, either: the argument loads are sunk across block
// boundaries, and each sunk group is a round trip of its own.  (Before: the atan copy was two exec-masked branches with a wait in
// each, then three argument loads with a wait each, then the table loads.  profiles/cells_prologue/README.md has the instruction
// listings and what the change measured.)
template <typename T, bool NT, int R>
__global__ __launch_bounds__(64 * R, 4) void k_cells_tile(GridK g, OutPtrs o, TileArgs ta)
{
    __shared__ __attribute__((aligned(16))) double atabs[R][TPG_ATAN_TABLE_DOUBLES];
    __shared__ TileLds<R> lds;
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // point row of this wave
    // one copy of the atan interval table per wave: needs no block barrier (LDS operations of one wave execute in order)
    double* atab = atabs[p];
    const unsigned long long atab_word = tpgb::atan_table_load(lane);       // round trip 1, with the kernel arguments
    const int tiles_x = ta.tiles_x, tiles = ta.tiles, grouped = ta.grouped;
    // Tiles are counted tx fastest, tile rows NORTH to SOUTH, so that the one slow row of a launch -- row Ny, whose wave takes the
    // general (scalar) path through coord(): +2.2 us of block latency -- starts first instead of ending the launch.  Worth ~0.3 % at
    // 1/10 degree (in-process A/B, round 4: 505.7 -> 504.2 us per build, i.e. inside the noise); kept because it costs nothing.
#if TPG_CELLS_PROBE == 4
    const int tiles_y = tiles / tiles_x;
#else
    const int tiles_y = ta.tiles_y;
#endif
    // columns: lanes 0-31 ascend from shift + 30 tx (lane 1 of tile 0 is f1 = shift + 1, the column of lambda = -180), lanes 32-63 hold
    // the Center images 2 shift + 1 - (column of lane 63 - l), ascending as well, so lane +- 1 is the east / west neighbour inside
    // each half; all wrapped into 1..Nx, every lane evaluates a valid column.  The pair index kk < Nx / 2 guards a partial last tile.
    const int hl = lane & 31;
    const double Rad = g.R;
    const bool fast_grid = absD(g.fplp90) <= 360.0;
#if TPG_CELLS_PROBE == 2 || TPG_CELLS_PROBE == 3
    unsigned long long fold = 0; unsigned fold_off = 0; bool folded = false;
#endif

    const int t = tpgt::tile_of_block((int)blockIdx.x, tiles, grouped != 0);
#if TPG_CELLS_PROBE == 4
    const int ty = tiles_y - 1 - t / tiles_x, tx = t % tiles_x;
#else
    const tpgt::TileXY txy = tpgt::tile_xy(t, tiles_x, tiles_y, ta.tiles_x_rcp);
    const int ty = txy.ty, tx = txy.tx;
#endif
    const int s0 = g.jm_lo - 1 + ty * (R - 1);
    const int s = s0 + p;                                                    // this wave's step
    // a select of two wave-uniform values as mask arithmetic: written as ?:, it becomes an exec-masked branch, and every branch in front
    // of the table loads is a block boundary that the loads of the arguments are sunk across
    const int colA = g.shift + 30 * tx, colB = g.shift - 30 * tx - 30;     // scalar
    const int icol = colA + ((colB - colA) & -(lane >> 5)) + hl;
    asm volatile("" :: "s"(g.ti), "s"(g.tj));                                // every argument of round trip 1 is loaded HERE, in the entry block
#if TPG_CELLS_PROBE == 4
    const int i = wrap_col_per_lane(icol, g.Nx);
#else
    const int i = tpgt::wrap_col(icol, g.Nx);
#endif
    LaneConst lc;
#if TPG_CELLS_PROBE == 3
    const RowTab rt = RowTab{ 0.5 + 1e-3 * (s & 7), 1.1, 0.6, 1.2 };
    lc.aslF = 0.31 + 0.01 * hl; lc.aclF = 0.72 + 1e-3 * (i & 1); lc.aslC = 0.33 + 0.01 * hl; lc.aclC = 0.74;
#else
    // round trip 2: the table entries
    RowTab rt = load_rowtab(g, s, s + 1);                                    // clamped: loaded whether or not the wave takes the fast path
#if TPG_CELLS_PROBE == 4
    lc.aslF = g.ti[0 * g.Nx + i - 1]; lc.aclF = g.ti[1 * g.Nx + i - 1];      // every lane's column is a valid one
    lc.aslC = g.ti[2 * g.Nx + i - 1]; lc.aclC = g.ti[3 * g.Nx + i - 1];
#else
    {
        // (uniform table base) + (32-bit unsigned byte offset in a VGPR), the saddr form, as the stores: i >= 1, and 32 Nx < 2^32 (the launcher checks)
        const char* ti = reinterpret_cast<const char*>(g.ti);
        const unsigned nx8 = 8u * (unsigned)g.Nx, i8 = 8u * (unsigned)(i - 1);
        auto at = [&](unsigned boff) -> double { return *reinterpret_cast<const double*>(ti + boff); };
        lc.aslF = at(i8); lc.aclF = at(i8 + nx8); lc.aslC = at(i8 + 2u * nx8); lc.aclC = at(i8 + 3u * nx8);
    }
#endif
#endif
#if TPG_CELLS_PROBE != 3
    // The psi entries are pinned HERE, in front of the store: left to the compiler, the four scalar loads are issued only behind the store
    // and its wait (a load from constant memory moves freely across the fences below, towards its reader).  The pin is no instruction but
    // it is a wait: for round trip 2, which the first product needs whole anyway.
    asm volatile("" : "+s"(rt.shC), "+s"(rt.chC), "+s"(rt.shF), "+s"(rt.chF));
#endif
    // the atan table goes to LDS now (LDS operations of one wave execute in order: no block barrier)
    tpgb::atan_table_store(atab, lane, atab_word);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#if TPG_CELLS_PROBE != 3
    // pins the lambda entries in front of the branch below (see "the prologue" above); no instruction, and the paired path's first
    // products read these registers next
    asm volatile("" : "+v"(lc.aslF), "+v"(lc.aclF), "+v"(lc.aslC), "+v"(lc.aclC));
#endif
    // no && here: a short-circuit is a branch per term
    const bool col_emit = ((unsigned)(hl - 1) < 30u) & (30 * tx + (lane >= 32 ? 30 - hl : hl - 1) < g.Nx / 2);
    const bool active_row = s <= g.jm_hi;                                    // rows past the band: idle waves
    const unsigned col = (unsigned)(i + g.Hx - 1);
    auto rowoff = [&](int j) -> unsigned { return (col + (unsigned)g.sx * (unsigned)(j - g.jstart + g.Hy)) * (unsigned)sizeof(T); };   // bytes

    // ---- phase 1: one point set per thread
    Step4 q;
    if (active_row) {
        // wave-uniform (TPG_RARE: always true in the ledger's scratch build).  s >= 0 always; row s = 0 -- the apron wave of the southernmost
        // tile row of a band that starts at row 1 -- is on the fast path too: its Face-y points FF(1), CF(1) are ordinary row-1 points,
        // and its Center-y points are the zero south halo, set below (the row table was loaded for the clamped row 1: any finite chain)
        const bool fast = !TPG_RARE(!(s < g.Ny && fast_grid));
        if (fast) {
            int i0 = i - g.shift; if (i0 < 1) i0 += g.Nx;
            lc.hemi = (i0 <= g.Nx / 2) ? -90.0 : 90.0;
#if TPG_CELLS_PROBE == 1
            const double pv = (lc.aslF + lc.aclC) * rt.shC + (double)(tx + lane);   // the table loads stay on the path
#pragma unroll
            for (int k = 0; k < 4; ++k) { q.lam[k] = pv; q.phi[k] = pv; q.a[k] = pv; q.ca[k] = pv; }
            q.X[0] = q.Y[0] = q.Z[0] = q.X[1] = q.Y[1] = q.Z[1] = pv;
#else
            points_pair<R>(g, lc, rt, q, atab, lds.v, p, lane);
#endif
        } else {
            Step4 tmp; GridK gc = g; points_general(gc, i, s, s + 1, tmp); q = tmp;
        }
        // coordinates: rows p >= 1 emit CC/FC(s) and FF/CF(s+1); the first tile's apron row emits FF/CF(jm_lo)
        if (col_emit) {
            if (p >= 1 && s >= g.jm_lo) {
                const unsigned off = pin_off(rowoff(s));
                TPG_EMIT_PINNED(TPG_LAMBDA_FC, off, q.lam[0]); TPG_EMIT_PINNED(TPG_PHI_FC, off, q.phi[0]);
                TPG_EMIT_PINNED(TPG_LAMBDA_CC, off, q.lam[1]); TPG_EMIT_PINNED(TPG_PHI_CC, off, q.phi[1]);
            }
            if ((p >= 1 || ty == 0) && s + 1 >= g.jm_lo && s + 1 <= g.jm_hi) {
                const unsigned off1 = pin_off(rowoff(s + 1));
                TPG_EMIT_PINNED(TPG_LAMBDA_FF, off1, q.lam[2]); TPG_EMIT_PINNED(TPG_PHI_FF, off1, q.phi[2]);
                TPG_EMIT_PINNED(TPG_LAMBDA_CF, off1, q.lam[3]); TPG_EMIT_PINNED(TPG_PHI_CF, off1, q.phi[3]);
            }
        }
        double (*L)[R][64] = lds.v;
        L[L_FC + 0][p][lane] = q.lam[0]; L[L_FC + 1][p][lane] = q.a[0]; L[L_FC + 2][p][lane] = q.ca[0];
        L[L_CC + 0][p][lane] = q.lam[1]; L[L_CC + 1][p][lane] = q.a[1]; L[L_CC + 2][p][lane] = q.ca[1];
        L[L_CC + 3][p][lane] = q.X[0];   L[L_CC + 4][p][lane] = q.Y[0]; L[L_CC + 5][p][lane] = q.Z[0];
        L[L_FF + 0][p][lane] = q.lam[2]; L[L_FF + 1][p][lane] = q.a[2]; L[L_FF + 2][p][lane] = q.ca[2];
        L[L_FF + 3][p][lane] = q.X[1];   L[L_FF + 4][p][lane] = q.Y[1]; L[L_FF + 5][p][lane] = q.Z[1];
        L[L_CF + 0][p][lane] = q.lam[3]; L[L_CF + 1][p][lane] = q.a[3]; L[L_CF + 2][p][lane] = q.ca[3];
        if (s == 0 && fast_grid) {
            // FC(0), CC(0) of the fast path: what coord() yields below row 1 -- (lambda, phi) = (0, 0), so a = 0 deg2rad = 0, cos(0) = 1
            // and the unit vector (cosd 0 cosd 0, sind 0 cosd 0, sind 0) = (1, +0, +0).  Row 0 is an apron row (p = 0): nothing of it is
            // emitted and phase 2 reads it from LDS only, so the records are overwritten here (LDS operations of a wave execute in order)
            // and not in q, where the merge would cost every wave its moves.  tests/test_cells_trims3.py holds them against k_cells.
            L[L_FC + 0][p][lane] = 0.0; L[L_FC + 1][p][lane] = 0.0; L[L_FC + 2][p][lane] = 1.0;
            L[L_CC + 0][p][lane] = 0.0; L[L_CC + 1][p][lane] = 0.0; L[L_CC + 2][p][lane] = 1.0;
            L[L_CC + 3][p][lane] = 1.0; L[L_CC + 4][p][lane] = 0.0; L[L_CC + 5][p][lane] = 0.0;
        }
    }
    __syncthreads();                                                         // the only barrier: point sets in LDS
    if (p == 0) {
        // The apron wave has no cell row of its own: instead of idling through phase 2 it computes one of the
        // eight haversines, Dy_ff = hav(FC(i,s), FC(i,s-1)), for every row of the tile from LDS (two rows at a time)
        if (col_emit) {
            double (*L)[R][64] = lds.v;
            // rows in pairs while two are left, then the odd one alone (a whole tile: three pairs and row R - 1), as the cell rows do
            // for Dy_cf: no haversine is evaluated twice
            int r = 1;
#pragma unroll 1
            for (; r + 1 < R && s0 + r + 1 <= g.jm_hi; r += 2) {
                const int sa = s0 + r, sb = sa + 1;
                double dd2[2];
#if TPG_CELLS_PROBE == 1
                dd2[0] = dd2[1] = L[L_FC + 0][r][lane];
#else
                Nb X[2] = { Nb{ L[L_FC + 0][r][lane], L[L_FC + 1][r][lane], L[L_FC + 2][r][lane] },
                            Nb{ L[L_FC + 0][r + 1][lane], L[L_FC + 1][r + 1][lane], L[L_FC + 2][r + 1][lane] } };
                Nb Y[2] = { Nb{ L[L_FC + 0][r - 1][lane], L[L_FC + 1][r - 1][lane], L[L_FC + 2][r - 1][lane] }, X[0] };
                hav_batch<2>(X, Y, Rad, dd2);
#endif
                if (sa >= g.jm_lo) TPG_EMIT(TPG_DY_FF, rowoff(sa), dd2[0]);
                if (sb >= g.jm_lo) TPG_EMIT(TPG_DY_FF, rowoff(sb), dd2[1]);
            }
            if (r < R && s0 + r <= g.jm_hi) {
                const int sa = s0 + r;
                double dd1[1];
#if TPG_CELLS_PROBE == 1
                dd1[0] = L[L_FC + 0][r][lane];
#else
                Nb X[1] = { Nb{ L[L_FC + 0][r][lane], L[L_FC + 1][r][lane], L[L_FC + 2][r][lane] } };
                Nb Y[1] = { Nb{ L[L_FC + 0][r - 1][lane], L[L_FC + 1][r - 1][lane], L[L_FC + 2][r - 1][lane] } };
                hav_batch<1>(X, Y, Rad, dd1);
#endif
                if (sa >= g.jm_lo) TPG_EMIT(TPG_DY_FF, rowoff(sa), dd1[0]);
            }
        }
    } else if (active_row && s >= g.jm_lo) {                                 // idle rows have no phase 2 (wave-uniform)
        if (col_emit) {                                                      // nor have apron lanes
        // ---- phase 2: the cell (i, s) from own registers + LDS neighbours, loaded just in time so that the
        //      live set stays under 128 VGPRs (4 waves/SIMD supply the ILP; batches of 2 suffice)
        // LDS addresses: one VGPR base per lane shift -- this lane, its east and its west neighbour, all at row p - 1 -- and the plane
        // f and the row (0: p - 1, 1: p) as the immediate offset of the read, (f R + row) * 512 B.  The bases are opaque to the compiler
        // (lds_base), so it pairs reads of one base across planes (ds_read2st64_b64, offsets in units of 512 B: any plane and row fits)
        // and not across lanes (ds_read2_b64 on lane, lane + 1 of one plane: 2040 B of reach, so a v_add_u32 per plane for a new base).
        // A single read reaches 65535 B: this lane and its west neighbour are read on planes 3 (L_CC) to 17 only, so their bases sit on
        // plane 2 and the planes 16, 17 need no second base.
        const int pm = p - 1;
        const LdsBase b0 = { lds_base(&lds.v[2][pm][lane]), 2 }, bW = { lds_base(&lds.v[2][pm][lane - 1]), 2 };
        const LdsBase bE = { lds_base(&lds.v[0][pm][lane + 1]), 0 };
        auto rd = [&](const LdsBase& b, int f, int row) -> double { return b.p[((f - b.plane) * R + row) * 64]; };
        const unsigned off = rowoff(s);
        double d[8];
#if TPG_CELLS_PROBE == 1
        {
            const double pv = q.lam[0] + rd(bE, L_FC + 0, 0);
            TPG_EMIT(TPG_AZ_CC, off, pv); TPG_EMIT(TPG_AZ_FF, off, pv);
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = pv;
        }
#else
        // 2 spherical quadrilaterals first (unit vectors only): Az_cc from FF points, Az_ff from CC points
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            V3 a, b, c, dd;
            if (k == 0) {   // ffP = FF(i,s), ffEP = FF(i+1,s), ffE = FF(i+1,s+1), ff = FF(i,s+1)
                a = V3{ rd(b0, L_FF + 3, 0), rd(b0, L_FF + 4, 0), rd(b0, L_FF + 5, 0) };
                b = V3{ rd(bE, L_FF + 3, 0), rd(bE, L_FF + 4, 0), rd(bE, L_FF + 5, 0) };
                c = V3{ rd(bE, L_FF + 3, 1), rd(bE, L_FF + 4, 1), rd(bE, L_FF + 5, 1) };
                dd = V3{ q.X[1], q.Y[1], q.Z[1] };
            } else {        // ccWP = CC(i-1,s-1), ccP = CC(i,s-1), cc = CC(i,s), ccW = CC(i-1,s)
                a = V3{ rd(bW, L_CC + 3, 0), rd(bW, L_CC + 4, 0), rd(bW, L_CC + 5, 0) };
                b = V3{ rd(b0, L_CC + 3, 0), rd(b0, L_CC + 4, 0), rd(b0, L_CC + 5, 0) };
                c = V3{ q.X[0], q.Y[0], q.Z[0] };
                dd = V3{ rd(bW, L_CC + 3, 1), rd(bW, L_CC + 4, 1), rd(bW, L_CC + 5, 1) };
            }
            double tt[4], at[4];
            // the four denominators of a cell finer than ~0.3 degrees are 4 (1 - d), 0 <= d < 2^-16: the division that starts from 1/4
            // instead of v_rcp_f64 (same bits); a wave with any other denominator divides as before (wave-uniform, like the atan tiers)
            {
                const double tn[4] = { tri_num(a, b, c), tri_num(a, b, dd), tri_num(a, c, dd), tri_num(b, c, dd) };
                const double td[4] = { tri_den(a, b, c), tri_den(a, b, dd), tri_den(a, c, dd), tri_den(b, c, dd) };
                if (__any(tpgb::div_near_b<4, true>(tn, td, tt))) {
                    tt[0] = tri_tan_nr(a, b, c); tt[1] = tri_tan_nr(a, b, dd);
                    tt[2] = tri_tan_nr(a, c, dd); tt[3] = tri_tan_nr(b, c, dd);
                }
            }
            // three tiers, each wave-uniform: +0 <= t < 2^-14 (every cell of a grid finer than ~0.9 degrees: the short exact form); the
            // full polynomial of before for a wave with a larger tangent (coarse grids, which run what they ran, behind one branch);
            // and the fallback for large, degenerate or negative triangles
            if (__any(tpgb::atan_tiny_b<4>(tt, at))) {
                if (__any(tpgb::atan_small_b<4, true>(tt, at))) {
                    tt[0] = tri_tan(a, b, c); tt[1] = tri_tan(a, b, dd); tt[2] = tri_tan(a, c, dd); tt[3] = tri_tan(b, c, dd);
                    tpgb::atan_b<4>(tt, at);
                }
            }
            // (2 t0 + 2 t1 + 2 t2 + 2 t3) / 2, summed left to right, is t0 + t1 + t2 + t3 summed left to right: doubling and halving are
            // exact and commute with every rounding (no overflow / underflow at these magnitudes) -- 5 multiplications less per quadrilateral
            double A = at[0];
            A += at[1];
            A += at[2];
            A += at[3];
            TPG_EMIT(k == 0 ? TPG_AZ_CC : TPG_AZ_FF, off, A * (Rad * Rad));
        }

        // 8 haversines in pairs; operand e = (x point, y point), each {lam, a, ca}
        //   0 dxcc(fcE,fc) 1 dxfc(cc,ccW) 2 dxcf(ffEP,ffP) 3 dxff(cfP,cfWP) 4 dycc(cf,cfP) 5 dyfc(ff,ffP) 6 dycf(cc,ccP) 7 dyff(fc,fcP)
        auto ld = [&](int f, int row, const LdsBase& b) -> Nb { return Nb{ rd(b, f + 0, row), rd(b, f + 1, row), rd(b, f + 2, row) }; };
        const Nb own[4] = { Nb{ q.lam[0], q.a[0], q.ca[0] }, Nb{ q.lam[1], q.a[1], q.ca[1] },
                            Nb{ q.lam[2], q.a[2], q.ca[2] }, Nb{ q.lam[3], q.a[3], q.ca[3] } };   // fc cc ff cf
#pragma unroll
        for (int hb = 0; hb < 6; hb += 2) {
            Nb X[2], Y[2];
            if (hb == 0)      { X[0] = ld(L_FC, 1, bE); Y[0] = own[0];          X[1] = own[1];          Y[1] = ld(L_CC, 1, bW); }
            else if (hb == 2) { X[0] = ld(L_FF, 0, bE); Y[0] = ld(L_FF, 0, b0); X[1] = ld(L_CF, 0, b0); Y[1] = ld(L_CF, 0, bW); }
            else              { X[0] = own[3];          Y[0] = ld(L_CF, 0, b0); X[1] = own[2];          Y[1] = ld(L_FF, 0, b0); }
            double dd2[2];
            hav_batch<2>(X, Y, Rad, dd2);
            d[hb] = dd2[0]; d[hb + 1] = dd2[1];
        }
        {   // Dy_cf here; Dy_ff is the apron wave's
            Nb X[1] = { own[1] }, Y[1] = { ld(L_CC, 0, b0) };
            double dd1[1];
            hav_batch<1>(X, Y, Rad, dd1);
            d[6] = dd1[0];
        }
#endif
        const unsigned offe = pin_off(off);                                  // the nine stores below are one basic block
        TPG_EMIT_PINNED(TPG_DX_CC, offe, d[0]); TPG_EMIT_PINNED(TPG_DX_FC, offe, d[1]);
        TPG_EMIT_PINNED(TPG_DX_CF, offe, d[2]); TPG_EMIT_PINNED(TPG_DX_FF, offe, d[3]);
        TPG_EMIT_PINNED(TPG_DY_CC, offe, d[4]); TPG_EMIT_PINNED(TPG_DY_FC, offe, d[5]);
        TPG_EMIT_PINNED(TPG_DY_CF, offe, d[6]);
        TPG_EMIT_PINNED(TPG_AZ_FC, offe, d[5] * d[1]);
        TPG_EMIT_PINNED(TPG_AZ_CF, offe, d[6] * d[2]);
        }
    }
#if TPG_CELLS_PROBE == 2 || TPG_CELLS_PROBE == 3
    if (folded) { put32<T, NT>(o, TPG_DX_CC, fold_off, __longlong_as_double((long long)fold)); folded = false; }
#endif
}
#undef TPG_EMIT
#undef TPG_EMIT_PINNED

// ---- K2: halo cells of the 20 arrays ------------------------------------------------------------
// x/y location of array q (order of enum tpg_array)
__device__ __forceinline__ void array_loc(int q, int& xl, int& yl)
{
    // cc, fc, cf, ff for every group except dy (cc, cf, fc, ff)
    int r = q & 3;
    bool dy = (q >= TPG_DY_CC && q <= TPG_DY_FF);
    int xr = dy ? (r >> 1) : (r & 1);
    int yr = dy ? (r & 1) : (r >> 1);
    xl = xr; yl = yr;
}

struct HaloRegions {
    int nA;   // x-halo columns of evaluated rows: (jm_hi-jm_lo+1) * 2Hx
    int nB;   // north rows j = Ny+1..jend+Hy present in the band (all Hy of them on the north rank)
    int nC;   // south rows j < 1 present in the band (+ row 1 when K3 is merged): (nsouth + row1) * sx
    int nD;   // row-Ny substitution cells i = Nx/2+1..Nx (bands that contain row Ny): Nx/2
    int nsouth;
    int merged_south;   // 1: this launch also writes the lat-lon continuation rows j <= 1 of the 12 metrics (K3)
};

template <typename T>
__global__ __launch_bounds__(256) void k_halos(GridK g, OutPtrs o, HaloRegions h)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int q = blockIdx.y;
    int xl, yl;
    array_loc(q, xl, yl);
    const bool is_coord = q < TPG_DX_CC;
    T* A = static_cast<T*>(o.p[q]);
    const long long sx = g.sx;
    auto at = [&](int i, int j) -> long long { return (long long)(i + g.Hx - 1) + sx * (j - g.jstart + g.Hy); };

    int i, j;
    if (t < h.nA) {
        int r = t / (2 * g.Hx), c = t - r * 2 * g.Hx;
        j = g.jm_lo + r;
        i = c < g.Hx ? 1 - g.Hx + c : g.Nx + 1 + (c - g.Hx);
        if (h.merged_south && !is_coord && j <= 1) return;   // row 1 of the metrics is written whole by region C
    } else if ((t -= h.nA) < h.nB) {
        int r = t / g.sx, c = t - r * g.sx;
        j = g.Ny + 1 + r; i = 1 - g.Hx + c;
    } else if ((t -= h.nB) < h.nC) {
        int r = t / g.sx, c = t - r * g.sx;
        j = 1 - h.nsouth + r; i = 1 - g.Hx + c;
        if (is_coord) { if (j < 1) A[at(i, j)] = (T)0; return; }   // south = nothing: halos stay zero (tripolar_grid.jl:148)
        if (!h.merged_south) return;             // metrics: rows j <= 1 belong to K3
        // continue_south! (tripolar_grid.jl:287-300,336-357): Dx and Az by y-location, one Dy for all
        const int n = g.Hy + 1, rt = j - (1 - g.Hy);
        const int col = (q >= TPG_DY_CC && q <= TPG_DY_FF) ? 4 : ((q >= TPG_AZ_CC ? 2 : 0) + (yl == TPG_FACE ? 1 : 0));
        A[at(i, j)] = (T)g.ts[col * n + rt];
        return;
    } else if ((t -= h.nC) < h.nD) {
        if (is_coord || yl != TPG_CENTER) return; // coordinates were evaluated through the substitution already
        i = g.Nx / 2 + 1 + t; j = g.Ny;
    } else {
        return;
    }

    int iw = i < 1 ? i + g.Nx : (i > g.Nx ? i - g.Nx : i);
    int js = j;
    if (j > g.Ny) {
        int dj = j - g.Ny;
        js = (yl == TPG_FACE) ? g.Ny - dj + 1 : g.Ny - dj;
        iw = fold_partner(xl, iw, g.Nx);
        if (js < 1) { A[at(i, j)] = (T)0; return; }     // folds a zero south-halo row (Ny <= Hy grids)
    } else if (j == g.Ny && yl == TPG_CENTER && iw > g.Nx / 2) {
        iw = fold_partner(xl, iw, g.Nx);
    }
    A[at(i, j)] = A[at(iw, js)];
}

// ---- K3: lat-lon continuation rows (continue_south!, src/tripolar_grid.jl:287-300,336-357) ----
template <typename T>
__global__ __launch_bounds__(256) void k_south(GridK g, OutPtrs o)
{
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    int r = blockIdx.y;                              // global row j = 1-Hy+r
    int lr = (1 - g.Hy + r) - (g.jstart - g.Hy);     // local row of the band
    if (c >= g.sx || lr < 0 || lr >= g.rows) return;
    int n = g.Hy + 1;
    double dxc = g.ts[0 * n + r], dxf = g.ts[1 * n + r], azc = g.ts[2 * n + r], azf = g.ts[3 * n + r], dy = g.ts[4 * n + r];
    long long off = (long long)c + (long long)g.sx * lr;
    put<T>(o, TPG_DX_FF, off, dxf); put<T>(o, TPG_DX_FC, off, dxc); put<T>(o, TPG_DX_CF, off, dxf); put<T>(o, TPG_DX_CC, off, dxc);
    put<T>(o, TPG_DY_FF, off, dy);  put<T>(o, TPG_DY_FC, off, dy);  put<T>(o, TPG_DY_CF, off, dy);  put<T>(o, TPG_DY_CC, off, dy);
    put<T>(o, TPG_AZ_FF, off, azf); put<T>(o, TPG_AZ_FC, off, azc); put<T>(o, TPG_AZ_CF, off, azf); put<T>(o, TPG_AZ_CC, off, azc);
}

size_t table_doubles(const tpg_params* p) { return 4 * (size_t)p->Nx + 4 * (size_t)p->Ny + 5 * (size_t)(p->Hy + 1); }

int check_params(const tpg_params* p)
{
    if (!p) { tpg::set_error("null params"); return TPG_ERR_INVALID_ARGUMENT; }
    int rc = tpg::check_geom(p->Nx, p->Ny, p->Nz, p->Hx, p->Hy, p->Hz, p->ft);
    if (rc) return rc;
    if (p->jstart < 1 || p->jend > p->Ny || p->jend < p->jstart) {
        tpg::set_error("latitude band %d:%d outside 1:%d", p->jstart, p->jend, p->Ny);
        return TPG_ERR_BAD_PARTITION;
    }
    if (p->reserved & ~TPG_BUILD_TABLES_VALID) {
        tpg::set_error("tpg_params.reserved: unknown flag bits 0x%x", p->reserved & ~TPG_BUILD_TABLES_VALID);
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (!(p->radius > 0) || !(p->north_poles_latitude < 90) || !(p->southernmost_latitude < 90)) {
        tpg::set_error("invalid radius / latitudes");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    return TPG_OK;
}

template <typename T>
int launch_build(const GridK& g, const OutPtrs& o, const HaloRegions& h, hipStream_t s)
{
    dim3 grid1(((g.Nx + 255) / 256) * (g.jm_hi - g.jm_lo + 1));
    // knobs (tpg::config(), read once; test library): TPG_CELLS_VARIANT 2 = k_cells_tile + k_halos (default, and the product's only form),
    // 0 = k_cells (thread per cell) + k_halos -- the cross-check: tests/test_gpu_variants.py; TPG_BUILD_NT 1 = streaming stores (default), 0 = plain
    // TPG_CELLS_ORDER 1 = XCD-grouped tile order (default, the product's), 0 = block id = tile (cross-check, A/B)
    const tpg::Config& cfg = tpg::config();
    const bool nt = cfg.build_nt;
    int rc = TPG_OK;
    constexpr int R = 8;                                       // point rows per tile (16 = one block per CU: measured 25 % slower)
    const int nrows = g.jm_hi - g.jm_lo + 1;
    const int tiles_y = (nrows + (R - 1) - 1) / (R - 1);
    const bool offsets32 = (unsigned long long)g.sx * (unsigned long long)(g.jend - g.jstart + 1 + 2 * g.Hy) * sizeof(T) < (1ull << 32);
    const bool south_in_band = g.jstart - g.Hy <= 1;
    const bool tables32 = g.Nx < (1 << 27) && g.Ny < (1 << 27);                    // the tile kernel reads its tables at 32-bit byte offsets: 4 x 8 Nx, 4 x 8 Ny
    const bool tile = cfg.cells_variant != 0 && tiles_y <= 65535 && offsets32 && tables32;     // the sizes that took the tile kernel when tile rows rode on gridDim.y; stores use 32-bit byte offsets
    if (tile) {
        const int tiles_x = (g.Nx / 2 + 29) / 30;                  // two strips of 30 emitting columns per wave: a lambda -> -lambda pair
        const int tiles = tiles_x * tiles_y;                       // far below 2^31: offsets32 bounds Nx x rows by 2^30, a tile emits up to 60 x 7 cells
        const TileArgs ta = { tiles_x, tiles, cfg.cells_order, tiles_y, tpgt::rcp_of((unsigned)tiles_x) };
        if (nt) hipLaunchKernelGGL((k_cells_tile<T, true, R>), dim3((unsigned)tiles), dim3(64 * R), 0, s, g, o, ta);
        else    hipLaunchKernelGGL((k_cells_tile<T, false, R>), dim3((unsigned)tiles), dim3(64 * R), 0, s, g, o, ta);
    }
    else if (nt) hipLaunchKernelGGL((k_cells<T, true>), grid1, dim3(256), 0, s, g, o);
    else         hipLaunchKernelGGL((k_cells<T, false>), grid1, dim3(256), 0, s, g, o);
    if ((rc = tpg::launch_status("k_cells"))) return rc;
    // K3 rides in the K2 launch unless the grid is so short that a north-fold source row or the row-Ny
    // substitution could be a continuation row (then K3 must run after K2, as in the reference's order)
    HaloRegions hm = h;
    hm.merged_south = (south_in_band && g.Ny > 2 * g.Hy + 2) ? 1 : 0;
    if (hm.merged_south) hm.nC = (h.nsouth + 1) * g.sx;
    int nh = hm.nA + hm.nB + hm.nC + hm.nD;
    if (nh > 0) {
        hipLaunchKernelGGL(k_halos<T>, dim3((nh + 255) / 256, TPG_NUM_ARRAYS), dim3(256), 0, s, g, o, hm);
        if ((rc = tpg::launch_status("k_halos"))) return rc;
    }
    if (south_in_band && !hm.merged_south) {
        hipLaunchKernelGGL(k_south<T>, dim3((g.sx + 255) / 256, g.Hy + 1), dim3(256), 0, s, g, o);
        if ((rc = tpg::launch_status("k_south"))) return rc;
    }
    return TPG_OK;
}

}  // namespace

extern "C" {

size_t tpg_build_grid_workspace_bytes(const tpg_params* p)
{
    if (!p || p->Nx < 1 || p->Ny < 1 || p->Hy < 0) return 0;
    return (table_doubles(p) * sizeof(double) + 255) & ~(size_t)255;
}

int tpg_build_grid(const tpg_params* p, void* const out[TPG_NUM_ARRAYS], void* workspace,
                   size_t workspace_bytes, void* stream)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!out) { tpg::set_error("null output table"); return TPG_ERR_INVALID_ARGUMENT; }
    OutPtrs o;
    for (int q = 0; q < TPG_NUM_ARRAYS; ++q) {
        if (!out[q]) { tpg::set_error("null output array %d", q); return TPG_ERR_INVALID_ARGUMENT; }
        o.p[q] = out[q];
    }
    if (!workspace || workspace_bytes < table_doubles(p) * sizeof(double) || ((uintptr_t)workspace & 7)) {
        tpg::set_error("workspace: need %zu bytes, 8-byte aligned", table_doubles(p) * sizeof(double));
        return TPG_ERR_WORKSPACE;
    }
    hipStream_t s = tpg::as_stream(stream);
    double* w = static_cast<double*>(workspace);

    TableArgs t;
    t.Nx = p->Nx; t.Ny = p->Ny; t.Hy = p->Hy; t.shift = p->Nx / 4; t.ft = p->ft;
    t.south = p->southernmost_latitude; t.npl = p->north_poles_latitude; t.R = p->radius;
    t.ti = w; t.tj = w + 4 * (size_t)p->Nx; t.ts = t.tj + 4 * (size_t)p->Ny;
    if (!(p->reserved & TPG_BUILD_TABLES_VALID)) {       // the caller may vouch for tables left in the workspace by an earlier call
        int nt = p->Nx + 2 * p->Ny + p->Hy + 1;
        hipLaunchKernelGGL(k_tables, dim3((nt + 63) / 64), dim3(64), 0, s, t);
        if ((rc = tpg::launch_status("k_tables"))) return rc;
    }

    GridK g;
    g.Nx = p->Nx; g.Ny = p->Ny; g.Hx = p->Hx; g.Hy = p->Hy; g.shift = p->Nx / 4;
    g.jstart = p->jstart; g.jend = p->jend;
    g.jm_lo = p->jstart - p->Hy < 1 ? 1 : p->jstart - p->Hy;
    g.jm_hi = p->jend + p->Hy > p->Ny ? p->Ny : p->jend + p->Hy;
    g.sx = p->Nx + 2 * p->Hx; g.rows = p->jend - p->jstart + 1 + 2 * p->Hy;
    g.ft = p->ft; g.fplp90 = p->first_pole_longitude + 90.0; g.R = p->radius;
    g.ti = t.ti; g.tj = t.tj; g.ts = t.ts;

    HaloRegions h;
    h.nA = (g.jm_hi - g.jm_lo + 1) * 2 * g.Hx;
    // north fold rows / row-Ny substitution: on the north rank, and on any band whose halo reaches them
    // (bands thinner than the halo: the reference slices them out of the global padded arrays)
    h.nB = (p->jend + p->Hy > p->Ny) ? (p->jend + p->Hy - p->Ny) * g.sx : 0;
    h.nsouth = (1 - (p->jstart - p->Hy)) > 0 ? (1 - (p->jstart - p->Hy)) : 0;   // rows j < 1 in the band
    h.nC = h.nsouth * g.sx;
    h.nD = (p->jend + p->Hy >= p->Ny) ? p->Nx / 2 : 0;

    if (p->ft == TPG_F64) return launch_build<double>(g, o, h, s);
    return launch_build<float>(g, o, h, s);
}

}  // extern "C"
