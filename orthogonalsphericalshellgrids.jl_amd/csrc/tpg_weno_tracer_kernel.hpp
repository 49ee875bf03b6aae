// tpg_weno_tracer_kernel.hpp -- the ONE kernel of the fifth-order WENO tracer tendencies and the ONE host launch of their two entry points:
// - !ZW: WENO5 in x and y, the centred mean in z (tpg_weno_tracer_advection_tendency, tpg_weno.hip; the rule: include/tripolar_hip_weno.h);
// - ZW: WENO5 in x, y AND z with walls in z (tpg_weno_xyz_tracer_advection_tendency, tpg_weno_xyz.hip; include/tripolar_hip_weno_xyz.h).
// `if constexpr (ZW)` wraps what only the z-window needs: there is no run-time branch on the form, and the statements of the x-y form are in
// the order they had before the two forms were one kernel.  The including file passes its compile-time switches as a type SW with JT (rows
// per work item), NT (G goes out in streaming stores), WAVES (waves per SIMD the register allocation must leave room for; 2: at most 256
// VGPRs), SHARE_X (the east-most x-flux of an item comes from the lane to the east, where Hx >= W), GROUP (the largest group of tracers a
// work item takes: 1, 2 or 4) and LOOKAHEAD (levels whose loads are in flight ahead of the arithmetic; 0: no ring): each library keeps its
// own -D names and defaults.  Evaluated in the field type T with no contraction; every operation is one correctly rounded IEEE operation.
// Each flux is formed once; where one is formed twice (tile edges) it has the same bits.
//
// Of the family of k_tracer_advection (tpg_advection.hip), written from the rule: a work item is ONE chunk of W interior columns x JT rows
// and walks ALL levels innermost (grid.y counts the tracers, or the tracer groups of a GROUP > 1 build).  It loads once the metrics and
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
// - Registers, x-y form.  Every kernel of the build stays within 256 VGPRs with no scratch, so that two waves share a SIMD:
//   __launch_bounds__(256, 2) and the build's resource usage (hipcc -Rpass-analysis=kernel-resource-usage: 153 - 234 VGPRs).  That budget
//   decides two things.  One tracer per item: groups of 2 or 4 sharing Mx, My, Mz, 1 / V spill at two waves and measure slower at one (the
//   shared products are a few per cent of a face's arithmetic).  No look-ahead ring: a level's loads go out at the level and the other wave
//   covers them; a ring of one level spills at two waves and measures slower at one.  Both stay compile-time switches.
//
// The z-window (ZW; one tracer per item and no ring: TG = 1, LA = 0).  At level K an item carries its own W x JT cells of c at the levels
// K-2 .. K+2 (win[0..4]; win[2] is the level's own row, the only slot of the x-y form, win[3] what that form fetches as the row one level up)
// and fetches level K+3: every c cell is still loaded ONCE for the vertical.  The plane of the look-ahead load is clamped onto plane Nz + 1,
// which exists since Hz >= 1: nothing beyond it is addressed, and what a clamped slot holds is never selected (the order table).  The class
// of the level's top face depends on the level only, so it is wave-uniform: a scalar branch, not a select across the four face values.
// The window adds three levels of W x JT cells to the registers above (profiles/weno_xyz/): 2 rows under __launch_bounds__(256, 1) --
// 246 - 252 VGPRs in Float64 and 166 - 262 in Float32, so two or three waves share a SIMD in every form but the Float32 16-B form without
// the shared x-flux -- are 13 % (Float64) and 20 % (Float32) faster than 1 row under (256, 2); 2 rows under (256, 2) spill 28 B in those
// four kernels and are not built.  No build may use scratch.  The level's loads of this form are written at their place in the level loop
// and not through `load`: the order in which a level's addresses and loads are written decides the registers, and through the lambdas the
// Float32 W = 2 SHARE kernels lose the third wave per SIMD (profiles/weno_tracer_kernel/).
#pragma once
#include "tpg_operator.hpp"
#include "tpg_tracer_tendency.hpp"
#include "tpg_weno_face.hpp"

namespace {

constexpr int HALO = 3;                    // cells a face reads on either side, whichever way the flow goes: c[i-3 .. i+2] around face i
constexpr int LANES = 64, CHUNKS_PER_WAVE = LANES - 1;   // SHARE: lane 63 only supplies a flux

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

// M * (M >= 0 ? R(x0, x1, x2, x3, x4) : R(x5, x4, x3, x2, x1)) for the six cells x0..x5 around the face between x2 and x3:
// five selects (true for -0, false for NaN), one evaluation of R (weno_face, tpg_weno_face.hpp: the one definition)
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

template <typename T, int W, bool GEN, bool MASK, int TG, int LA, bool SHARE, bool ZW, typename SW>
__global__ __launch_bounds__(256, SW::WAVES) void k_weno_tracer_advection(TracerPtrs p, WenoArgs a)
{
    static_assert(!ZW || (TG == 1 && LA == 0), "the z-window is built for one tracer per item and without a ring");
    typedef Chunk<T, W, GEN> cvec_t;
    constexpr int JT = SW::JT;
    constexpr int NF = SHARE ? W : W + 1;                          // x-faces an item forms per row: the west faces of its columns (+ its east-most)
    constexpr int NE = NF + 2 - W;                                 // elements east of the chunk the x-faces read: face f reads columns f-3 .. f+2
    constexpr int WIN = ZW ? 5 : 1, C = WIN / 2;                   // levels of the z-window an item carries (ZW: K-2 .. K+2 at level K) and its centre slot
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
    const T* c[TG];                                                // level 1 of the tile's first cell; level L is L - 1 planes up
    T* G[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        c[t] = static_cast<const T*>(p.c[q0 + t]) + f0;
        G[t] = static_cast<T*>(p.G[q0 + t]) + f0;
    }
    const T mv = (T)a.value;

    struct Tracer {
        cvec_t ca[JT], cs[HALO], cn[HALO];                         // c one level up (ZW: three); the three rows south and north of the tile at this level
        T cw[JT][HALO], ce[JT][NE];                                // c three elements west and NE east of each row at this level
    };
    struct Level {
        cvec_t u[JT], v[JT + 1], w[JT];                            // w at the level's TOP face
        T ue[JT], d;                                               // (ue: the plain form only)
        Tracer tr[LA > 0 ? TG : 1];                                // (in the ring and ZW only: otherwise a tracer's cells are loaded at its turn)
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

    // carried from level to level: the z-window of c (win[C]: the c rows of the level; ZW: win[s] is level K - 2 + s, the slots below level 1
    // hold level 1 and are never selected) and Fz at the level's bottom face (the top face of the level below).  ZW: level L <= Nz + 1 sits
    // min(L - 1, Nz) planes above level 1: the clamp keeps every address on or below plane Nz + 1.
    T win[TG][WIN][JT][W], fzb[TG][JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t w1 = *reinterpret_cast<const cvec_t*>(w + ro[r]);
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            const cvec_t c1 = *reinterpret_cast<const cvec_t*>(c[t] + rc[r + HALO]);
            const cvec_t c0 = *reinterpret_cast<const cvec_t*>(c[t] - a.plane + rc[r + HALO]);   // the bottom halo plane
#pragma unroll
            for (int s = 0; s <= C; ++s)
#pragma unroll
                for (int e = 0; e < W; ++e) win[t][s][r][e] = c1[e];
#pragma unroll
            for (int s = C + 1; s < WIN; ++s) {
                const cvec_t cu = *reinterpret_cast<const cvec_t*>(c[t] + a.plane * min(s - C, a.Nz) + rc[r + HALO]);
#pragma unroll
                for (int e = 0; e < W; ++e) win[t][s][r][e] = cu[e];
            }
#pragma unroll
            for (int e = 0; e < W; ++e) fzb[t][r][e] = (azr[r][e] * w1[e]) * (T(0.5) * (c0[e] + c1[e]));
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
            if constexpr (ZW) {
                // u, v, w at the level's TOP face, the c rows three levels up, the three rows south and north of the tile and the elements
                // west and east of each row at this level, in THIS order (the opening comment)
                Level& L = ring[s];
                Tracer& X = L.tr[0];
                const T* uk = u + a.plane * k;
                const T* vk = v + a.plane * k;
                const T* wk = w + a.plane * (k + 1);
                const T* ck = c[0] + a.plane * k;
                const T* cf = c[0] + a.plane * min(k + 3, a.Nz);   // level K + 3 = k + 4, clamped onto plane Nz + 1
                L.d = dz[k];
#pragma unroll
                for (int r = 0; r < JT; ++r) {
                    L.u[r] = *reinterpret_cast<const cvec_t*>(uk + ro[r]);
                    if constexpr (!SHARE) L.ue[r] = uk[ro[r] + W];
                    L.w[r] = *reinterpret_cast<const cvec_t*>(wk + ro[r]);
                    X.ca[r] = *reinterpret_cast<const cvec_t*>(cf + rc[r + HALO]);
#pragma unroll
                    for (int q = 0; q < HALO; ++q) X.cw[r][q] = ck[rc[r + HALO] - HALO + q];
#pragma unroll
                    for (int q = 0; q < NE; ++q) X.ce[r][q] = ck[rc[r + HALO] + eo[q]];
                }
#pragma unroll
                for (int r = 0; r <= JT; ++r) L.v[r] = *reinterpret_cast<const cvec_t*>(vk + ro[r]);
#pragma unroll
                for (int q = 0; q < HALO; ++q) {
                    X.cs[q] = *reinterpret_cast<const cvec_t*>(ck + rc[q]);
                    X.cn[q] = *reinterpret_cast<const cvec_t*>(ck + rc[JT + HALO + q]);
                }
            } else {
                if constexpr (LA == 0) load(ring[s], k);
            }
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
                if constexpr (LA > 0 || ZW) X = L.tr[t];
                else load_tracer(X, t, k);
                // ZW: Fz at the level's top face, face k + 2 (1-based): its class is the level's, the same in every lane
                T fzw[JT][W];
                if constexpr (ZW) {
                    const T (&n)[WIN][JT][W] = win[t];
                    const int cls = weno_z_face_class(k + 2, a.Nz);
                    if (cls == WENO_Z_ORDER5) {
#pragma unroll
                        for (int r = 0; r < JT; ++r)
#pragma unroll
                            for (int e = 0; e < W; ++e)
                                fzw[r][e] = upwind_flux<T>(mz[r][e], n[0][r][e], n[1][r][e], n[2][r][e], n[3][r][e], n[4][r][e], X.ca[r][e]);
                    } else if (cls == WENO_Z_ORDER3) {
#pragma unroll
                        for (int r = 0; r < JT; ++r)
#pragma unroll
                            for (int e = 0; e < W; ++e) fzw[r][e] = upwind_flux3<T>(mz[r][e], n[1][r][e], n[2][r][e], n[3][r][e], n[4][r][e]);
                    } else if (cls == WENO_Z_ORDER1) {
#pragma unroll
                        for (int r = 0; r < JT; ++r)
#pragma unroll
                            for (int e = 0; e < W; ++e) fzw[r][e] = mz[r][e] * (mz[r][e] >= T(0) ? n[2][r][e] : n[3][r][e]);
                    } else {
#pragma unroll
                        for (int r = 0; r < JT; ++r)
#pragma unroll
                            for (int e = 0; e < W; ++e) fzw[r][e] = mz[r][e] * (T(0.5) * (n[2][r][e] + n[3][r][e]));
                    }
                }
                // Fy at the JT + 1 y-faces of each column: the column's cells from three rows south of the tile to three rows north of it
                T fy[JT + 1][W];
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    T cy[JT + 2 * HALO];
#pragma unroll
                    for (int s = 0; s < HALO; ++s) { cy[s] = X.cs[s][e]; cy[JT + HALO + s] = X.cn[s][e]; }
#pragma unroll
                    for (int r = 0; r < JT; ++r) cy[HALO + r] = win[t][C][r][e];
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
                    for (int e = 0; e < W; ++e) cx[HALO + e] = win[t][C][r][e];
#pragma unroll
                    for (int s = 0; s < NE; ++s) cx[HALO + W + s] = X.ce[r][s];
#pragma unroll
                    for (int f = 0; f < NF; ++f) fx[f] = upwind_flux<T>(mx[r][f], cx[f], cx[f + 1], cx[f + 2], cx[f + 3], cx[f + 4], cx[f + 5]);
                    if constexpr (SHARE) fx[W] = __shfl_down(fx[0], 1);       // the west-most flux of the chunk to the east: this chunk's east-most
                    cvec_t out;
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        T fzt;
                        if constexpr (ZW) fzt = fzw[r][e];
                        else fzt = mz[r][e] * (T(0.5) * (win[t][C][r][e] + X.ca[r][e]));
                        const T g = -(rV[r][e] * (((fx[e + 1] - fx[e]) + (fy[r + 1][e] - fy[r][e])) + (fzt - fzb[t][r][e])));
                        fzb[t][r][e] = fzt;
                        out[e] = (MASK && k < m[r][e]) ? mv : g;
                    }
                    if (r < nr && !ghost) store_chunk<SW::NT>(reinterpret_cast<cvec_t*>(G[t] + a.plane * k + a.sx * r), out);
                }
                // the window moves one level up
#pragma unroll
                for (int r = 0; r < JT; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) {
#pragma unroll
                        for (int s = 0; s + 1 < WIN; ++s) win[t][s][r][e] = win[t][s + 1][r][e];
                        win[t][WIN - 1][r][e] = X.ca[r][e];
                    }
            }
        }
    }
}

// the launch of both entry points, after tpg::check_geom and TracerCall::check: the work-item bound, the Args, the chunk form, the SHARE
// form where the chunk past a row's end lies inside the east halo, the mask, and one launch per group size (tracer_groups<1>: ONE launch)
template <bool ZW, typename SW>
int launch_weno_tracers(const TracerCall& call, double mask_value, const char* name, void* stream)
{
    const Geom& g = call.g;
    const long long tiles = (g.Ny + SW::JT - 1) / SW::JT;
    const long long widest = (long long)(g.Nx / 2 + CHUNKS_PER_WAVE - 1) / CHUNKS_PER_WAVE * LANES;    // threads per row tile, at most: the SHARE form with W = 2
    if (tiles * widest >= (1ll << 31) - 256) { tpg::set_error("tracer advection: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    const TracerPtrs p = call.pointers();
    void* arrays[2 * TPG_MAX_FIELDS + 6];
    const int na = call.arrays(arrays);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(call.ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = g.Nx / cp.W;
        const bool share = SW::SHARE_X && g.Hx >= cp.W;            // the chunk past a row's end lies inside the east halo
        const int wpr = (cpr + CHUNKS_PER_WAVE - 1) / CHUNKS_PER_WAVE;   // a wave stores 63 chunks; the last one's lane after the last chunk takes the chunk past the end
        WenoArgs a{ g.Nx, g.Ny, g.Nz, g.sx, 0, cpr, wpr, (int)tiles, (int)(share ? tiles * wpr * LANES : tiles * cpr), g.plane, interior2(g), interior3(g),
                    call.n_cc ? (double)(T)mask_value : 0.0 };
        const unsigned blocks = (unsigned)((a.items + 255) / 256);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto launch = [&](auto mask, auto sh) {
                constexpr bool MASK = decltype(mask)::value;
                constexpr bool SHARE = decltype(sh)::value;
                tracer_groups<SW::GROUP>(call.nfields, [&](auto tg, int q0, int n) {
                    a.q0 = q0;
                    hipLaunchKernelGGL((k_weno_tracer_advection<T, W, GEN, MASK, decltype(tg)::value, SW::LOOKAHEAD, SHARE, ZW, SW>), dim3(blocks, n), dim3(256), 0,
                                       st, p, a);
                });
            };
            auto by_mask = [&](auto sh) {
                if (call.n_cc) launch(std::true_type{}, sh);
                else           launch(std::false_type{}, sh);
            };
            if constexpr (SW::SHARE_X) { if (share) { by_mask(std::true_type{}); return; } }
            by_mask(std::false_type{});
        });
        return tpg::launch_status(name);
    });
}

}  // namespace
