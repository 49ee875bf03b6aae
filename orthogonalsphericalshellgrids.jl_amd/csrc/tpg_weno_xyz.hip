// tpg_weno_xyz.hip -- the flux-form advection tendency of the tracers at (Center, Center, Center) with a fifth-order WENO reconstruction in
// x, y AND z, for gfx950 (tpg_weno_xyz_tracer_advection_tendency): the scheme `WENO()` of the reference's distributed driver, and like
// tpg_weno_tracer_advection_tendency's result the Gn of the AB2 step of the tracers.
// [recalled: Oceananigans' WENO() = FluxFormAdvection(WENO(order = 5) x3) on a z-Bounded grid; parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_weno_xyz.h: x and y are include/tripolar_hip_weno.h's (R5 = weno_face of
// tpg_weno_face.hpp, five selects and ONE evaluation per face); a z-face takes the centred mean at the two walls, the upwind cell one face
// away from a wall, R3 (weno_face3) two faces away and R5 from three on, whichever way the flow goes.  Evaluated in the field type T, in
// exactly that order, with no contraction; every operation is one correctly rounded IEEE operation.
// - Cells read: c[-2..Nx+3, j, k], c[i, -2..Ny+3, k], c[i, j, 0..Nz+1] (no corner halo cell, no z-halo plane but 0 and Nz + 1 at any Hz);
//   u[1..Nx+1, j, k], v[i, 1..Ny+1, k], w[i, j, 1..Nz+1]; the same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.
// - Only interior cells of G are written.  Mask and several tracers: as in tpg_weno_tracer_advection_tendency.
//
// Of the family of k_weno_tracer_advection (tpg_weno.hip), whose work item, chunk forms, SHARE form of the x-flux, ghost lane, clamped rows,
// fused mask and streaming stores carry over: a work item is ONE chunk of W interior columns x JT rows and walks ALL levels innermost, one
// tracer per item (grid.y counts the tracers), a level's loads going out at the level.  New is the z-window.  At level K an item carries its
// own W x JT cells of c at the levels K-2 .. K+2 (win[0..4]; win[2] is the level's own row, what that kernel calls cc, win[3] its ca) and
// fetches level K+3: every c cell is still loaded ONCE for the vertical.  The plane of the look-ahead load is clamped onto plane Nz + 1,
// which exists since Hz >= 1: nothing beyond it is addressed, and what a clamped slot holds is never selected (the order table).  Fz at the
// level's bottom face is carried as before.  The class of the level's top face depends on the level only, so it is wave-uniform: a scalar
// branch, not a select across the four face values.
//
// Registers decide the form (profiles/weno_xyz/): the window adds three levels of W x JT cells to a kernel that stood at 153 - 234 of 256
// VGPRs.  TPG_WXYZ_JT rows per item at TPG_WXYZ_WAVES waves per SIMD are compile-time; no build may use scratch.  Measured at
// 3600 x 1800 x 75, alternating: 2 rows under __launch_bounds__(256, 1) -- 246 - 252 VGPRs in Float64 and 166 - 262 in Float32, so two or
// three waves share a SIMD in every form but the Float32 16-B form without the shared x-flux -- are 13 % (Float64) and 20 % (Float32) faster
// than 1 row under (256, 2); 2 rows under (256, 2) spill 28 B in those four kernels and are not built.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "tpg_tracer_tendency.hpp"
#include "tpg_weno_face.hpp"
#include "../../include/tripolar_hip_weno_xyz.h"

// compile-time switches of the A/B in profiles/weno_xyz/ (make WENO_XYZ_TAG=_jt2w1 WENO_XYZ_FLAGS='-DTPG_WXYZ_JT=2 -DTPG_WXYZ_WAVES=1',
// -DTPG_WXYZ_SHARE=0 or -DTPG_WXYZ_NT=0).  What was measured at 3600 x 1800 x 75 and why these are the defaults: DESIGN.md 6, profiles/weno_xyz/.
#ifndef TPG_WXYZ_JT
#define TPG_WXYZ_JT 2
#endif
#ifndef TPG_WXYZ_WAVES
#define TPG_WXYZ_WAVES 1
#endif
#ifndef TPG_WXYZ_SHARE
#define TPG_WXYZ_SHARE 1
#endif
#ifndef TPG_WXYZ_NT
#define TPG_WXYZ_NT 1
#endif

namespace {

constexpr int JT = TPG_WXYZ_JT;            // rows per work item
constexpr int WAVES = TPG_WXYZ_WAVES;      // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)
constexpr bool SHARE_X = TPG_WXYZ_SHARE;   // the east-most x-flux of an item comes from the lane to the east (where Hx >= W)
constexpr bool NT = TPG_WXYZ_NT;           // G goes out in streaming stores
constexpr int HALO = 3;                    // cells a face reads on either side, whichever way the flow goes: c[i-3 .. i+2] around face i
constexpr int LANES = 64, CHUNKS_PER_WAVE = LANES - 1;   // SHARE: lane 63 only supplies a flux
constexpr int WIN = 5;                     // levels of the z-window an item carries: K-2 .. K+2 at level K

struct WenoXyzPtrs {
    const void* c[TPG_MAX_FIELDS];
    void* G[TPG_MAX_FIELDS];
    const void *u, *v, *w;
    const void *dy, *dx, *az, *dz;
    const int32_t* ncc;
};

struct WenoXyzArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int wpr;                               // SHARE: waves per row tile
    int tiles;                             // row tiles
    int items;                             // threads with work: tiles x cpr, or (SHARE) tiles x wpr x 64
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double value;                          // the mask value (a T value held in a double)
};

// M * (M >= 0 ? R5(x0, x1, x2, x3, x4) : R5(x5, x4, x3, x2, x1)) for the six cells x0..x5 around the face between x2 and x3:
// five selects (true for -0, false for NaN), one evaluation of R5
template <typename T>
__device__ __forceinline__ T upwind_flux(T M, T x0, T x1, T x2, T x3, T x4, T x5)
{
    const bool pos = M >= T(0);
    return M * weno_face<T>(pos ? x0 : x5, pos ? x1 : x4, pos ? x2 : x3, pos ? x3 : x2, pos ? x4 : x1);
}

// M * (M >= 0 ? R3(x0, x1, x2) : R3(x3, x2, x1)) for the four cells x0..x3 around the face between x1 and x2
template <typename T>
__device__ __forceinline__ T upwind_flux3(T M, T x0, T x1, T x2, T x3)
{
    const bool pos = M >= T(0);
    return M * weno_face3<T>(pos ? x0 : x3, pos ? x1 : x2, pos ? x2 : x1);
}

template <typename T, int W, bool GEN, bool MASK, bool SHARE>
__global__ __launch_bounds__(256, WAVES) void k_weno_xyz_tracer_advection(WenoXyzPtrs p, WenoXyzArgs a)
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
    const int q = blockIdx.y;                                      // the tracer

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
    const T* c = static_cast<const T*>(p.c[q]) + f0;               // level 1 of the tile's first cell; level L is L - 1 planes up
    T* G = static_cast<T*>(p.G[q]) + f0;
    const T mv = (T)a.value;

    // carried from level to level: the z-window of c (win[s]: level K - 2 + s of the rows of the tile; the slots below level 1 hold level 1,
    // and are never selected) and Fz at the level's bottom face (the top face of the level below).  Level L <= Nz + 1 sits min(L - 1, Nz)
    // planes above level 1: the clamp keeps every address on or below plane Nz + 1.
    T win[WIN][JT][W], fzb[JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t w1 = *reinterpret_cast<const cvec_t*>(w + ro[r]);
        const cvec_t c0 = *reinterpret_cast<const cvec_t*>(c - a.plane + rc[r + HALO]);      // the bottom halo plane
        const cvec_t c1 = *reinterpret_cast<const cvec_t*>(c + rc[r + HALO]);
        const cvec_t c2 = *reinterpret_cast<const cvec_t*>(c + a.plane * min(1, a.Nz) + rc[r + HALO]);
        const cvec_t c3 = *reinterpret_cast<const cvec_t*>(c + a.plane * min(2, a.Nz) + rc[r + HALO]);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            win[0][r][e] = c1[e]; win[1][r][e] = c1[e]; win[2][r][e] = c1[e]; win[3][r][e] = c2[e]; win[4][r][e] = c3[e];
            fzb[r][e] = (azr[r][e] * w1[e]) * (T(0.5) * (c0[e] + c1[e]));
        }
    }

    for (int k = 0; k < a.Nz; ++k) {
        // the level's loads: u, v, w at the level's TOP face, the c rows three levels up, the three rows south and north of the tile and the
        // elements west and east of each row at this level.  No load depends on the previous level.
        const T* uk = u + a.plane * k;
        const T* vk = v + a.plane * k;
        const T* wk = w + a.plane * (k + 1);
        const T* ck = c + a.plane * k;
        const T* cf = c + a.plane * min(k + 3, a.Nz);              // level K + 3 = k + 4, clamped onto plane Nz + 1
        const T d = dz[k];
        cvec_t Lu[JT], Lv[JT + 1], Lw[JT], cnew[JT], cs[HALO], cn[HALO];
        T ue[JT], cw[JT][HALO], ce[JT][NE];
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            Lu[r] = *reinterpret_cast<const cvec_t*>(uk + ro[r]);
            if constexpr (!SHARE) ue[r] = uk[ro[r] + W];           // u[i + 1, j, k] of the chunk's last column
            Lw[r] = *reinterpret_cast<const cvec_t*>(wk + ro[r]);
            cnew[r] = *reinterpret_cast<const cvec_t*>(cf + rc[r + HALO]);
#pragma unroll
            for (int s = 0; s < HALO; ++s) cw[r][s] = ck[rc[r + HALO] - HALO + s];
#pragma unroll
            for (int s = 0; s < NE; ++s) ce[r][s] = ck[rc[r + HALO] + eo[s]];
        }
#pragma unroll
        for (int r = 0; r <= JT; ++r) Lv[r] = *reinterpret_cast<const cvec_t*>(vk + ro[r]);
#pragma unroll
        for (int s = 0; s < HALO; ++s) {
            cs[s] = *reinterpret_cast<const cvec_t*>(ck + rc[s]);                            // rows -3, -2, -1 of the tile
            cn[s] = *reinterpret_cast<const cvec_t*>(ck + rc[JT + HALO + s]);                // rows JT, JT + 1, JT + 2
        }

        T my[JT + 1][W], mx[JT][NF], mz[JT][W], rV[JT][W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
#pragma unroll
            for (int r = 0; r <= JT; ++r) my[r][e] = (dxr[r][e] * d) * Lv[r][e];
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                mx[r][e] = (dyc[r][e] * d) * Lu[r][e];
                mz[r][e] = azr[r][e] * Lw[r][e];
                rV[r][e] = T(1) / (azr[r][e] * d);
            }
        }
        if constexpr (!SHARE) {
#pragma unroll
            for (int r = 0; r < JT; ++r) mx[r][W] = (dyc[r][W] * d) * ue[r];
        }

        // Fz at the level's top face, face k + 2 (1-based): its class is the level's, the same in every lane
        T fzt[JT][W];
        const int cls = weno_z_face_class(k + 2, a.Nz);
        if (cls == WENO_Z_ORDER5) {
#pragma unroll
            for (int r = 0; r < JT; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e)
                    fzt[r][e] = upwind_flux<T>(mz[r][e], win[0][r][e], win[1][r][e], win[2][r][e], win[3][r][e], win[4][r][e], cnew[r][e]);
        } else if (cls == WENO_Z_ORDER3) {
#pragma unroll
            for (int r = 0; r < JT; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e) fzt[r][e] = upwind_flux3<T>(mz[r][e], win[1][r][e], win[2][r][e], win[3][r][e], win[4][r][e]);
        } else if (cls == WENO_Z_ORDER1) {
#pragma unroll
            for (int r = 0; r < JT; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e) fzt[r][e] = mz[r][e] * (mz[r][e] >= T(0) ? win[2][r][e] : win[3][r][e]);
        } else {
#pragma unroll
            for (int r = 0; r < JT; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e) fzt[r][e] = mz[r][e] * (T(0.5) * (win[2][r][e] + win[3][r][e]));
        }

        // Fy at the JT + 1 y-faces of each column: the column's cells from three rows south of the tile to three rows north of it
        T fy[JT + 1][W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            T cy[JT + 2 * HALO];
#pragma unroll
            for (int s = 0; s < HALO; ++s) { cy[s] = cs[s][e]; cy[JT + HALO + s] = cn[s][e]; }
#pragma unroll
            for (int r = 0; r < JT; ++r) cy[HALO + r] = win[2][r][e];
#pragma unroll
            for (int r = 0; r <= JT; ++r) fy[r][e] = upwind_flux<T>(my[r][e], cy[r], cy[r + 1], cy[r + 2], cy[r + 3], cy[r + 4], cy[r + 5]);
        }
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            // Fx at the row's x-faces: the row from three elements west of the chunk to NE east of it
            T cx[W + HALO + NE], fx[W + 1];
#pragma unroll
            for (int s = 0; s < HALO; ++s) cx[s] = cw[r][s];
#pragma unroll
            for (int e = 0; e < W; ++e) cx[HALO + e] = win[2][r][e];
#pragma unroll
            for (int s = 0; s < NE; ++s) cx[HALO + W + s] = ce[r][s];
#pragma unroll
            for (int f = 0; f < NF; ++f) fx[f] = upwind_flux<T>(mx[r][f], cx[f], cx[f + 1], cx[f + 2], cx[f + 3], cx[f + 4], cx[f + 5]);
            if constexpr (SHARE) fx[W] = __shfl_down(fx[0], 1);           // the west-most flux of the chunk to the east: this chunk's east-most
            cvec_t out;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const T g = -(rV[r][e] * (((fx[e + 1] - fx[e]) + (fy[r + 1][e] - fy[r][e])) + (fzt[r][e] - fzb[r][e])));
                fzb[r][e] = fzt[r][e];
                out[e] = (MASK && k < m[r][e]) ? mv : g;
            }
            if (r < nr && !ghost) store_chunk<NT>(reinterpret_cast<cvec_t*>(G + a.plane * k + a.sx * r), out);
        }
        // the window moves one level up
#pragma unroll
        for (int r = 0; r < JT; ++r)
#pragma unroll
            for (int e = 0; e < W; ++e) {
#pragma unroll
                for (int s = 0; s + 1 < WIN; ++s) win[s][r][e] = win[s + 1][r][e];
                win[WIN - 1][r][e] = cnew[r][e];
            }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_weno_xyz_last_error(void) { return tpg_last_error(); }

int tpg_weno_xyz_tracer_advection_tendency(const void* const* c, void* const* G, int nfields, const void* u, const void* v, const void* w,
                                           const void* dy_fc, const void* dx_cf, const void* az_cc, const void* dz_c, const int32_t* n_cc,
                                           double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    const TracerCall call{ c, G, nfields, u, v, w, dy_fc, dx_cf, az_cc, dz_c, n_cc, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft };
    if (int rc = call.check(HALO, 1, "c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1]")) return rc;
    const Geom& g = call.g;
    const long long tiles = (Ny + JT - 1) / JT;
    const long long widest = (long long)(Nx / 2 + CHUNKS_PER_WAVE - 1) / CHUNKS_PER_WAVE * LANES;      // threads per row tile, at most: the SHARE form with W = 2
    if (tiles * widest >= (1ll << 31) - 256) { tpg::set_error("tracer advection: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    const WenoXyzPtrs p = call.pointers<WenoXyzPtrs>();
    void* arrays[2 * TPG_MAX_FIELDS + 6];
    const int na = call.arrays(arrays);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        const bool share = SHARE_X && Hx >= cp.W;                  // the chunk past a row's end lies inside the east halo
        const int wpr = (cpr + CHUNKS_PER_WAVE - 1) / CHUNKS_PER_WAVE;   // a wave stores 63 chunks; the last one's lane after the last chunk takes the chunk past the end
        const WenoXyzArgs a{ Nx, Ny, Nz, g.sx, cpr, wpr, (int)tiles, (int)(share ? tiles * wpr * LANES : tiles * cpr), g.plane, interior2(g), interior3(g),
                             n_cc ? (double)(T)mask_value : 0.0 };
        const unsigned blocks = (unsigned)((a.items + 255) / 256);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto launch = [&](auto mask, auto sh) {
                hipLaunchKernelGGL((k_weno_xyz_tracer_advection<T, W, GEN, decltype(mask)::value, decltype(sh)::value>), dim3(blocks, nfields), dim3(256), 0, st,
                                   p, a);
            };
            auto by_mask = [&](auto sh) {
                if (n_cc) launch(std::true_type{}, sh);
                else      launch(std::false_type{}, sh);
            };
            if constexpr (SHARE_X) { if (share) { by_mask(std::true_type{}); return; } }
            by_mask(std::false_type{});
        });
        return tpg::launch_status("k_weno_xyz_tracer_advection");
    });
}

}  // extern "C"
