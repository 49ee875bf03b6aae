// tpg_weno.hip -- the flux-form advection tendency of the tracers at (Center, Center, Center) with a fifth-order WENO reconstruction in x
// and y and the centred mean in z, for gfx950 (tpg_weno_tracer_advection_tendency): the scheme of the reference's drivers, and like
// tpg_tracer_advection_tendency's result the Gn of the AB2 step of the tracers.
// [recalled: Oceananigans' FluxFormAdvection(WENO(order = 5), WENO(order = 5), Centered()), uniform-grid coefficients, Jiang-Shu smoothness
// indicators, WENO-Z weights, eps = 1e-8; parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_weno.h: R(q0..q4) (weno_face of tpg_weno_face.hpp, operation for operation), the selection
// Mx >= 0 ? R(c[i-3..i+1]) : R(c[i+2..i-2]) (upwind_flux below: five selects, ONE evaluation of R per face), Mx, My, Mz, V, Fz and the last
// line those of tpg_tracer_advection_tendency.  Evaluated in the field type T, in exactly that order, with no contraction; every operation
// is one correctly rounded IEEE operation.  Each flux is formed once; where one is formed twice (tile edges) it has the same bits.
// - Cells read: c[-2..Nx+3, j, k], c[i, -2..Ny+3, k], c[i, j, 0..Nz+1] (a plus-shaped stencil, no corner halo cell); u[1..Nx+1, j, k],
//   v[i, 1..Ny+1, k], w[i, j, 1..Nz+1]; the same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.  So Hx >= 3, Hy >= 3, Hz >= 1.
// - Only interior cells of G are written.  Mask and several tracers: as in tpg_tracer_advection_tendency.
//
// Of the family of k_tracer_advection (tpg_advection.hip), written from the rule: a work item is ONE chunk of W interior columns x JT rows
// and walks ALL levels innermost (grid.y counts the tracers, or the tracer groups of a -DTPG_WENO_TG build).  It loads once the metrics and
// counts of the tile, carries from level to level Fz at the level's bottom face and the c rows of the level, and per level fetches u, v, w,
// the c rows one level up, the three rows south and the three rows north of the tile, and three elements west and east of each row.  No
// load depends on the previous level.  Rows of the last tile past the interior compute on clamped row offsets (inside the north halo) and
// store nothing.
//
// Unlike that kernel this one is VALU-bound (profiles/weno/): a face costs about sixty operations and four divisions.  So the design is
// about faces and registers, not streams:
// - Redundant faces.  An item of W columns x JT rows evaluates JT + 1 y-faces per column, and W + 1 x-faces per row -- or, in the SHARE
//   form, W: the east-most x-flux of a row comes from the lane to the east, which formed it as its west-most (the same bits).  There a
//   wave takes 63 chunks of one row tile and its lane 63 repeats the first chunk of the next wave (or the chunk past the row's end) only to
//   supply that flux: it stores nothing.  The chunk past the row's end sits in the east halo, so the SHARE form needs Hx >= W; a geometry
//   without that takes the plain form.  Measured: SHARE 14 % (Float64) and 6 % (Float32) faster than the plain form, 2 rows 13 - 16 % faster
//   than 1; 4 rows do not fit two waves per SIMD and are slower at one.
// - The select.  Five v_cndmask-style selects per face on Mx >= 0 (upwind_flux), no branch.
// - Registers.  Every kernel of the build stays within 256 VGPRs with no scratch, so that two waves share a SIMD: __launch_bounds__(256, 2)
//   and the build's resource usage (hipcc -Rpass-analysis=kernel-resource-usage: 153 - 234 VGPRs).  That budget decides two things.  One
//   tracer per item: groups of 2 or 4 sharing Mx, My, Mz, 1 / V spill at two waves and measure slower at one (the shared products are a
//   few per cent of a face's arithmetic).  No look-ahead ring: a level's loads go out at the level and the other wave covers them; a ring of
//   one level spills at two waves and measures slower at one.  Both stay compile-time switches.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "tpg_tracer_tendency.hpp"
#include "tpg_weno_face.hpp"
#include "../../include/tripolar_hip_weno.h"

// compile-time switches of the A/B in profiles/weno/ (make WENO_TAG=_jt1 WENO_FLAGS=-DTPG_WENO_JT=1, -DTPG_WENO_SHARE=0, -DTPG_WENO_TG=2,
// -DTPG_WENO_LOOKAHEAD=1, -DTPG_WENO_NT=0 or -DTPG_WENO_WAVES=1).  What was measured at 3600 x 1800 x 75 and why these are the defaults:
// DESIGN.md 6, profiles/weno/.
#ifndef TPG_WENO_TG
#define TPG_WENO_TG 1
#endif
#ifndef TPG_WENO_JT
#define TPG_WENO_JT 2
#endif
#ifndef TPG_WENO_SHARE
#define TPG_WENO_SHARE 1
#endif
#ifndef TPG_WENO_LOOKAHEAD
#define TPG_WENO_LOOKAHEAD 0
#endif
#ifndef TPG_WENO_NT
#define TPG_WENO_NT 1
#endif
#ifndef TPG_WENO_WAVES
#define TPG_WENO_WAVES 2
#endif

namespace {

constexpr int GROUP = TPG_WENO_TG;         // the largest group of tracers a work item takes, sharing Mx, My, Mz: 1 (no grouped kernel), 2 or 4
constexpr int JT = TPG_WENO_JT;            // rows per work item
constexpr bool SHARE_X = TPG_WENO_SHARE;   // the east-most x-flux of an item comes from the lane to the east (where Hx >= W)
constexpr int LOOKAHEAD = TPG_WENO_LOOKAHEAD;   // levels whose loads are in flight ahead of the arithmetic (0: no ring)
constexpr bool NT = TPG_WENO_NT;           // G goes out in streaming stores
constexpr int WAVES = TPG_WENO_WAVES;      // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)
constexpr int HALO = 3;                    // cells a face reads on either side, whichever way the flow goes: c[i-3 .. i+2] around face i
constexpr int LANES = 64, CHUNKS_PER_WAVE = LANES - 1;   // SHARE: lane 63 only supplies a flux

struct WenoPtrs {
    const void* c[TPG_MAX_FIELDS];
    void* G[TPG_MAX_FIELDS];
    const void *u, *v, *w;
    const void *dy, *dx, *az, *dz;
    const int32_t* ncc;
};

struct WenoArgs {
    int Nx, Ny, Nz, sx;
    int q0;                                // the launch's first tracer
    int cpr;                               // chunks per interior row
    int wpr;                               // SHARE: waves per row tile
    int tiles;                             // row tiles
    int items;                             // threads with work: tiles x cpr, or (SHARE) tiles x wpr x 64
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double value;                          // the mask value (a T value held in a double)
};

// R(q0, q1, q2, q3, q4) of the rule is weno_face (tpg_weno_face.hpp: the one definition, shared with tpg_weno_momentum.hip)

// M * (M >= 0 ? R(x0, x1, x2, x3, x4) : R(x5, x4, x3, x2, x1)) for the six cells x0..x5 around the face between x2 and x3:
// five selects (true for -0, false for NaN), one evaluation of R
template <typename T>
__device__ __forceinline__ T upwind_flux(T M, T x0, T x1, T x2, T x3, T x4, T x5)
{
    const bool pos = M >= T(0);
    return M * weno_face<T>(pos ? x0 : x5, pos ? x1 : x4, pos ? x2 : x3, pos ? x3 : x2, pos ? x4 : x1);
}

template <typename T, int W, bool GEN, bool MASK, int TG, int LA, bool SHARE>
__global__ __launch_bounds__(256, WAVES) void k_weno_tracer_advection(WenoPtrs p, WenoArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    constexpr int NF = SHARE ? W : W + 1;                          // x-faces an item forms per row: the west faces of its columns (+ its east-most)
    constexpr int NE = NF + 2 - W;                                 // elements east of the chunk the x-faces read: face f reads columns f-3 .. f+2
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    int tile, ch;
    bool ghost = false, past = false;
    if constexpr (SHARE) {
        const int wave = item / LANES, lane = item % LANES;
        tile = wave / a.wpr;
        ch = (wave - tile * a.wpr) * CHUNKS_PER_WAVE + lane;
        if (ch > a.cpr) return;
        past = ch == a.cpr;                                        // the chunk past the row's end, columns Nx .. Nx + W - 1 of the east halo (Hx >= W)
        ghost = past || lane == LANES - 1;                         // forms its west-most x-flux for the lane to the west, stores nothing
    } else {
        tile = item / a.cpr;
        ch = item - tile * a.cpr;
    }
    const int e0 = ch * W;                                         // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const int q0 = a.q0 + blockIdx.y * TG;                         // first tracer of the group

    // row offsets inside a plane.  ro: the tile's rows and the row north of the last, clamped onto the row north of the last interior one
    // (u, v, w, the metrics).  rc[r + 3]: rows -3 .. JT + 2 of the tile for c, clamped onto the third row north of the last interior one
    // (row j0 + nr + 2 <= Ny + 2, 0-based: inside the north halo, Hy >= 3); row j0 - 3 >= -3 is inside the south halo.
    int ro[JT + 1], rc[JT + 2 * HALO];
#pragma unroll
    for (int r = 0; r <= JT; ++r) ro[r] = a.sx * min(r, nr);
#pragma unroll
    for (int r = -HALO; r < JT + HALO; ++r) rc[r + HALO] = a.sx * min(r, nr + HALO - 1);
    // the elements east of the chunk: W .. W + NE - 1.  Of the chunk past the row's end only face 0 is used, which reads up to element 2
    // (column Nx + 2 <= Nx + Hx - 1): beyond that it re-reads its own first column instead, so that no address leaves the row
    int eo[NE];
#pragma unroll
    for (int s = 0; s < NE; ++s) eo[s] = past && W + s > HALO - 1 ? 0 : W + s;

    // the tile's metrics, once
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    const T* dy = static_cast<const T*>(p.dy) + m0;
    const T* dx = static_cast<const T*>(p.dx) + m0;
    const T* az = static_cast<const T*>(p.az) + m0;
    T dyc[JT][NF], dxr[JT + 1][W], azr[JT][W];
    int m[JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t y = *reinterpret_cast<const cvec_t*>(dy + ro[r]);
        const cvec_t z = *reinterpret_cast<const cvec_t*>(az + ro[r]);
        if constexpr (!SHARE) dyc[r][W] = dy[ro[r] + W];           // dy_fc[i + 1, j] of the chunk's last column
#pragma unroll
        for (int e = 0; e < W; ++e) { dyc[r][e] = y[e]; azr[r][e] = z[e]; m[r][e] = 0; }
        if constexpr (MASK) {                                      // a count plane has no halo: clamped onto the last interior row, and the chunk past the row's end onto column 0
            const Counts<W> n = *reinterpret_cast<const Counts<W>*>(p.ncc + (long long)a.Nx * (j0 + min(r, nr - 1)) + (past ? 0 : e0));
#pragma unroll
            for (int e = 0; e < W; ++e) m[r][e] = min(max(n[e], 0), a.Nz);   // masked levels (0-based k < m)
        }
    }
#pragma unroll
    for (int r = 0; r <= JT; ++r) {
        const cvec_t x = *reinterpret_cast<const cvec_t*>(dx + ro[r]);                        // rows j0 .. j0 + JT
#pragma unroll
        for (int e = 0; e < W; ++e) dxr[r][e] = x[e];
    }

    const long long f0 = a.off3 + (long long)a.sx * j0 + e0;
    const T* u = static_cast<const T*>(p.u) + f0;
    const T* v = static_cast<const T*>(p.v) + f0;
    const T* w = static_cast<const T*>(p.w) + f0;                  // face 1 of the tile's first cell; face k + 1 is one plane up per level
    const T* dz = static_cast<const T*>(p.dz);
    const T* c[TG];
    T* G[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        c[t] = static_cast<const T*>(p.c[q0 + t]) + f0;
        G[t] = static_cast<T*>(p.G[q0 + t]) + f0;
    }
    const T mv = (T)a.value;

    struct Tracer {
        cvec_t ca[JT], cs[HALO], cn[HALO];                         // c one level up; the three rows south and north of the tile at this level
        T cw[JT][HALO], ce[JT][NE];                                // c three elements west and NE east of each row at this level
    };
    struct Level {
        cvec_t u[JT], v[JT + 1], w[JT];                            // w at the level's TOP face
        T ue[JT], d;                                               // (ue: the plain form only)
        Tracer tr[LA > 0 ? TG : 1];                                // (in the ring only: without one a tracer's cells are loaded at its turn)
    };
    auto load_tracer = [&](Tracer& X, int t, int k) {
        const T* ck = c[t] + a.plane * k;
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            X.ca[r] = *reinterpret_cast<const cvec_t*>(ck + a.plane + rc[r + HALO]);
#pragma unroll
            for (int s = 0; s < HALO; ++s) X.cw[r][s] = ck[rc[r + HALO] - HALO + s];
#pragma unroll
            for (int s = 0; s < NE; ++s) X.ce[r][s] = ck[rc[r + HALO] + eo[s]];
        }
#pragma unroll
        for (int s = 0; s < HALO; ++s) {
            X.cs[s] = *reinterpret_cast<const cvec_t*>(ck + rc[s]);                            // rows -3, -2, -1 of the tile
            X.cn[s] = *reinterpret_cast<const cvec_t*>(ck + rc[JT + HALO + s]);                // rows JT, JT + 1, JT + 2
        }
    };
    auto load = [&](Level& L, int k) {
        const T* uk = u + a.plane * k;
        const T* vk = v + a.plane * k;
        const T* wk = w + a.plane * (k + 1);
        L.d = dz[k];
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            L.u[r] = *reinterpret_cast<const cvec_t*>(uk + ro[r]);
            if constexpr (!SHARE) L.ue[r] = uk[ro[r] + W];         // u[i + 1, j, k] of the chunk's last column
            L.w[r] = *reinterpret_cast<const cvec_t*>(wk + ro[r]);
        }
#pragma unroll
        for (int r = 0; r <= JT; ++r) L.v[r] = *reinterpret_cast<const cvec_t*>(vk + ro[r]);
        if constexpr (LA > 0) {
#pragma unroll
            for (int t = 0; t < TG; ++t) load_tracer(L.tr[t], t, k);
        }
    };

    // carried from level to level: the c rows of the level and Fz at its bottom face (the top face of the level below)
    T cc[TG][JT][W], fzb[TG][JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t w1 = *reinterpret_cast<const cvec_t*>(w + ro[r]);
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            const cvec_t c1 = *reinterpret_cast<const cvec_t*>(c[t] + rc[r + HALO]);
            const cvec_t c0 = *reinterpret_cast<const cvec_t*>(c[t] - a.plane + rc[r + HALO]);   // the bottom halo plane
#pragma unroll
            for (int e = 0; e < W; ++e) {
                cc[t][r][e] = c1[e];
                fzb[t][r][e] = (azr[r][e] * w1[e]) * (T(0.5) * (c0[e] + c1[e]));
            }
        }
    }

    constexpr int RING = LA > 0 ? LA : 1;                          // LA = 0: no ring, a level's loads go out at the level
    Level ring[RING];
    if constexpr (LA > 0) {
#pragma unroll
        for (int s = 0; s < RING; ++s) load(ring[s], min(s, a.Nz - 1));
    }
    for (int k0 = 0; k0 < a.Nz; k0 += RING) {
#pragma unroll
        for (int s = 0; s < RING; ++s) {
            const int k = k0 + s;
            if (k >= a.Nz) break;
            if constexpr (LA == 0) load(ring[s], k);
            const Level L = ring[s];
            if constexpr (LA > 0) { if (k + LA < a.Nz) load(ring[s], k + LA); }   // the loads of level k + LA go out before level k's arithmetic
            const T d = L.d;
            T my[JT + 1][W], mx[JT][NF], mz[JT][W], rV[JT][W];
#pragma unroll
            for (int e = 0; e < W; ++e) {
#pragma unroll
                for (int r = 0; r <= JT; ++r) my[r][e] = (dxr[r][e] * d) * L.v[r][e];
#pragma unroll
                for (int r = 0; r < JT; ++r) {
                    mx[r][e] = (dyc[r][e] * d) * L.u[r][e];
                    mz[r][e] = azr[r][e] * L.w[r][e];
                    rV[r][e] = T(1) / (azr[r][e] * d);
                }
            }
            if constexpr (!SHARE) {
#pragma unroll
                for (int r = 0; r < JT; ++r) mx[r][W] = (dyc[r][W] * d) * L.ue[r];
            }
#pragma unroll
            for (int t = 0; t < TG; ++t) {
                Tracer X;
                if constexpr (LA > 0) X = L.tr[t];
                else load_tracer(X, t, k);
                // Fy at the JT + 1 y-faces of each column: the column's cells from three rows south of the tile to three rows north of it
                T fy[JT + 1][W];
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    T cy[JT + 2 * HALO];
#pragma unroll
                    for (int s = 0; s < HALO; ++s) { cy[s] = X.cs[s][e]; cy[JT + HALO + s] = X.cn[s][e]; }
#pragma unroll
                    for (int r = 0; r < JT; ++r) cy[HALO + r] = cc[t][r][e];
#pragma unroll
                    for (int r = 0; r <= JT; ++r) fy[r][e] = upwind_flux<T>(my[r][e], cy[r], cy[r + 1], cy[r + 2], cy[r + 3], cy[r + 4], cy[r + 5]);
                }
#pragma unroll
                for (int r = 0; r < JT; ++r) {
                    // Fx at the row's x-faces: the row from three elements west of the chunk to NE east of it
                    T cx[W + HALO + NE], fx[W + 1];
#pragma unroll
                    for (int s = 0; s < HALO; ++s) cx[s] = X.cw[r][s];
#pragma unroll
                    for (int e = 0; e < W; ++e) cx[HALO + e] = cc[t][r][e];
#pragma unroll
                    for (int s = 0; s < NE; ++s) cx[HALO + W + s] = X.ce[r][s];
#pragma unroll
                    for (int f = 0; f < NF; ++f) fx[f] = upwind_flux<T>(mx[r][f], cx[f], cx[f + 1], cx[f + 2], cx[f + 3], cx[f + 4], cx[f + 5]);
                    if constexpr (SHARE) fx[W] = __shfl_down(fx[0], 1);       // the west-most flux of the chunk to the east: this chunk's east-most
                    cvec_t out;
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const T fzt = mz[r][e] * (T(0.5) * (cc[t][r][e] + X.ca[r][e]));
                        const T g = -(rV[r][e] * (((fx[e + 1] - fx[e]) + (fy[r + 1][e] - fy[r][e])) + (fzt - fzb[t][r][e])));
                        fzb[t][r][e] = fzt;
                        out[e] = (MASK && k < m[r][e]) ? mv : g;
                    }
                    if (r < nr && !ghost) store_chunk<NT>(reinterpret_cast<cvec_t*>(G[t] + a.plane * k + a.sx * r), out);
                }
#pragma unroll
                for (int r = 0; r < JT; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) cc[t][r][e] = X.ca[r][e];
            }
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_weno_last_error(void) { return tpg_last_error(); }

int tpg_weno_tracer_advection_tendency(const void* const* c, void* const* G, int nfields, const void* u, const void* v, const void* w,
                                       const void* dy_fc, const void* dx_cf, const void* az_cc, const void* dz_c, const int32_t* n_cc,
                                       double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    const TracerCall call{ c, G, nfields, u, v, w, dy_fc, dx_cf, az_cc, dz_c, n_cc, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft };
    if (int rc = call.check(HALO, 1, "c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-1..k+1]")) return rc;
    const Geom& g = call.g;
    const long long tiles = (Ny + JT - 1) / JT;
    const long long widest = (long long)(Nx / 2 + CHUNKS_PER_WAVE - 1) / CHUNKS_PER_WAVE * LANES;      // threads per row tile, at most: the SHARE form with W = 2
    if (tiles * widest >= (1ll << 31) - 256) { tpg::set_error("tracer advection: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    const WenoPtrs p = call.pointers<WenoPtrs>();
    void* arrays[2 * TPG_MAX_FIELDS + 6];
    const int na = call.arrays(arrays);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        const bool share = SHARE_X && Hx >= cp.W;                  // the chunk past a row's end lies inside the east halo
        const int wpr = (cpr + CHUNKS_PER_WAVE - 1) / CHUNKS_PER_WAVE;   // a wave stores 63 chunks; the last one's lane after the last chunk takes the chunk past the end
        WenoArgs a{ Nx, Ny, Nz, g.sx, 0, cpr, wpr, (int)tiles, (int)(share ? tiles * wpr * LANES : tiles * cpr), g.plane, interior2(g), interior3(g),
                    n_cc ? (double)(T)mask_value : 0.0 };
        const unsigned blocks = (unsigned)((a.items + 255) / 256);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto launch = [&](auto mask, auto sh) {
                constexpr bool MASK = decltype(mask)::value;
                constexpr bool SHARE = decltype(sh)::value;
                tracer_groups<GROUP>(nfields, [&](auto tg, int q0, int n) {
                    a.q0 = q0;
                    hipLaunchKernelGGL((k_weno_tracer_advection<T, W, GEN, MASK, decltype(tg)::value, LOOKAHEAD, SHARE>), dim3(blocks, n), dim3(256), 0, st, p, a);
                });
            };
            auto by_mask = [&](auto sh) {
                if (n_cc) launch(std::true_type{}, sh);
                else      launch(std::false_type{}, sh);
            };
            if constexpr (SHARE_X) { if (share) { by_mask(std::true_type{}); return; } }
            by_mask(std::false_type{});
        });
        return tpg::launch_status("k_weno_tracer_advection");
    });
}

}  // extern "C"
