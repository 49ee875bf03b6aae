// tpg_weno_vorticity_kernel.hpp -- the ONE kernel that forms the WENO5-upwinded vorticity flux of the momentum tendencies,
//     hu = -(vhat * zr), vhat = vh / dx_fc, zr = vhat >= 0 ? W5(Z[i, j-2 .. j+2]) : W5(Z[i, j+3 .. j-1])
//     hv =   uhat * zr,  uhat = uh / dy_cf, zr = uhat >= 0 ? W5(Z[i-2 .. i+2, j]) : W5(Z[i+3 .. i-1, j])
// (the rule: include/tripolar_hip_weno_momentum.h), in two forms chosen at compile time (FULL):
// - FULL: the whole tendency of tpg_weno_momentum_advection_tendency (tpg_weno_momentum.hip), -((hu + vu) + bu) and -((hv + vv) + bv) with
//   the centred vertical term and kinetic-energy gradient of k_momentum_advection (tpg_momentum.hip), masked;
// - !FULL: the vorticity term only, hu -> Gu and hv -> Gv, unmasked: the first launch of tpg_weno_vi_momentum_advection_tendency
//   (tpg_weno_vi.hip).  Nothing of w, dz, az_cc, az_fc, az_cf, the count planes, K, S, R, the rows one level up or the carried rows is
//   loaded or formed; the item loads all rows -3 .. JT + 2 of u (v: from -2) at its own level.
// `if constexpr (FULL)` wraps what only the whole tendency needs: there is no run-time branch on the form, and the statements of the FULL
// form are in the order they had before the two forms were one kernel.  The vorticity-only form has two `else` branches of its own, both
// loads: dy_fc without az_cc, and the level's rows of u and v.  The including file passes its compile-time switches as a type SW
// with SHARE (the Z beside the chunk come from the neighbouring lanes), NT (Gu, Gv go out in streaming stores), WAVES (waves per SIMD
// the register allocation must leave room for; 2: at most 256 VGPRs) and VS (the smoothness of the reconstruction is measured on the
// velocities, below): each library keeps its own -D names and defaults.
// W5 = weno_face (tpg_weno_face.hpp, the one definition): five selects on the sign (true for -0, false for NaN), ONE evaluation of W5 per
// node and direction.  Evaluated in the field type T with no contraction; every operation is one correctly rounded IEEE operation.
//
// ONE launch for both fields, of the family of k_momentum_advection (tpg_momentum.hip), written from the rule: a work item is ONE chunk of W
// interior columns x JT rows and walks ALL levels innermost.  It loads once the cells of the eight metric planes its nodes read and the count
// values, and keeps them in registers.  It carries from level to level S and R at the level's bottom face and the u, v rows of the level.  Per
// level: dz_f of the top face, the JT rows of u and v one level up, the rows -3 .. -1 and JT .. JT + 2 of the tile of u (v: from -2) on the
// chunk's columns, the element west of each row of v, the elements west and east of the tile's rows of u, and w at the top face.  No load
// depends on the previous level: the loads of the next LOOKAHEAD levels are issued before the current level's arithmetic (a ring of register
// slots).  Items are numbered (row tile, chunk) with the chunk fastest, 256 to a block.  Rows of the last tile past the interior compute on
// row offsets clamped onto row Ny + 3 (inside the north halo) and store nothing.
//
// What is new against that kernel is the cost of Z: a six-point window of a derived quantity (each Z ends in a division) in both directions.
// - y.  An item forms Z once on its own W columns at the rows -2 .. JT + 2 of its tile: JT + 5 values per column serve the JT windows of Gu.
//   So rows per item decide the cost: 6 Z per node and column at JT = 1, 3.5 at JT = 2.
// - x.  The windows of Gv need Z at the tile's rows on the columns -2, -1 and W .. W + 2 beside the chunk.  Those are the own columns of the
//   lanes west and east of it (one lane west; one east, two with W = 2): three or four cross-lane moves per row (__shfl_up / __shfl_down), no
//   LDS, no barrier.  Formed naively a 2 x 2 item would need 24 Z per level; this one forms 14.
// - wave edges.  A lane whose neighbour is not in its wave, not in its row tile, or past the row's end (the periodic seam: the halo columns
//   -2, -1 and Nx .. Nx + 2) forms those Z itself, with the same operations on element loads (zeta_at: the same bits) -- lanes 0, 62 and 63 of
//   every wave at least.  Unlike the tracer kernel's supplier lanes (tpg_weno_tracer_kernel.hpp, 63 chunks a wave), no lane is given up and no chunk lies
//   outside the interior: a supplier chunk of W = 4 columns beside the seam would read column -5 or Nx + 4, outside a row of halo 3 or 4, while
//   zeta_at reads exactly the cells of the rule.  The wave pays the divergent piece (at most 5 Z per row) once per level.
// - SW::SHARE = false is the naive form in x (every item forms its five neighbour Z per row by zeta_at); profiles/weno_momentum/.
// A second design -- a block-wide 2-D tile of Z in double-buffered LDS -- is recorded in profiles/weno_momentum/README.md and not built.
//
// Resources of the FULL form (gfx950 code object metadata of the build, profiles/weno_momentum/resources.json): 438 - 444 VGPRs in Float64
// (182 - 188 of them AGPRs), 420 - 424 in Float32 with 4-wide chunks and 276 with 2-wide ones; no scratch, no LDS; ONE wave per SIMD like
// k_momentum_advection -- the metric cells of the two crosses alone are 50 values per item.  Chosen by measurement at 3600 x 1800 x 75
// (profiles/weno_momentum/): 2 rows per item (1 row 11 % / 5 % slower, Float64 / Float32), no look-ahead ring (with 2 rows a ring of one level
// spills; with 1 row it is slower than none), the shared Z (13 % / 2 % faster than every item forming its own), streaming stores (4 % / 3 %).
// The vorticity-only form: profiles/vorticity_kernel/README.md.
//
// SW::VS (tpg_weno_vs.hip only, with !FULL only): the VelocityStencil form, the rule of include/tripolar_hip_weno_vs.h.  zr is W5V
// (weno_face_vs, tpg_weno_face.hpp) of the same Z window and the windows of
//     UB[i,j,k] = T(0.5) * (u[i,j-1,k] + u[i,j,k])   and   VB[i,j,k] = T(0.5) * (v[i-1,j,k] + v[i,j,k])
// at the nodes of the Z: fifteen selects, ONE evaluation per node and direction.  Everything else is the form above, statement for statement.
// [recalled: Oceananigans' biased WENO weights for VelocityStencil -- the smoothness indicators of the tangential stencils of the two
// velocities averaged onto (Face, Face), summed and halved (beta_sum); parity unpinned, like every operator here]
// - y.  UB and VB on the item's own columns at the rows -2 .. JT + 2 come from the rows of u and v the item holds for Z: no load is new.
// - x.  UB and VB of the tile's rows on the columns -2, -1 and W .. W + 2 are the neighbouring lanes' own.  Every lane forms them itself
//   from element loads (ub_at, vb_at: the same operations, the same bits, and exactly the elements of u and v that zeta_at reads for the Z
//   of that node -- no address is new); with SW::SHARE_VS they are moved across lanes beside Z instead and only a lane at a wave edge, a
//   row end or the seam forms them.  The loads won the A/B (5 % / 3 % of the call, Float64 / Float32): profiles/weno_vs/, with the resources.
#pragma once
#include "tpg_momentum_tendency.hpp"
#include "tpg_weno_face.hpp"

namespace {

constexpr int HALO = 3;                    // cells a window reads beyond the interior, whichever way the flow goes
constexpr int LANES = 64;

// Rows of the tile are r = -3 .. JT + 2 (r = 0 .. JT - 1 its own), columns c = -1 .. W (c = 0 .. W - 1 the chunk's).  The arrays with the
// two crosses (u, v, dxfc, dycf, azff) are indexed [r + 3][c + 1] ([r + 3][c] where no column -1 is read), the others as in
// k_momentum_advection.  Entries the rule does not read are never loaded and never used.
template <typename T, int W, bool GEN, bool MASK, int JT, int LA, typename SW, bool FULL>
__global__ __launch_bounds__(256, SW::WAVES) void k_weno_momentum_advection(MomentumPtrs p, MomentumArgs a)
{
    static_assert(FULL || !MASK, "the vorticity term alone is stored unmasked");
    static_assert(!(FULL && SW::VS), "VelocityStencil smoothness is built for the vorticity term alone");
    typedef Chunk<T, W, GEN> cvec_t;
    constexpr int NR = JT + 2 * HALO;                              // rows -3 .. JT + 2
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int ch = item - tile * a.cpr;
    const int e0 = ch * W;                                         // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const int lane = threadIdx.x % LANES;
    // the lane west (east, second east) of this one holds the chunk west (east, second east) of this one, of the same row tile
    const bool west_ok = SW::SHARE && lane > 0 && ch > 0;
    const bool east1_ok = SW::SHARE && lane < LANES - 1 && ch < a.cpr - 1;
    const bool east2_ok = SW::SHARE && lane < LANES - 2 && ch < a.cpr - 2;
    const T half = T(0.5);

    // row offsets inside a plane, rows -3 .. JT + 2 of the tile: the rows past the interior clamped onto the third row north of the last
    // interior one (row j0 + nr + 2 <= Ny + 2, 0-based: inside the north halo, Hy >= 3); row j0 - 3 >= -3 is inside the south halo
    int ro[NR];
#pragma unroll
    for (int r = -HALO; r < JT + HALO; ++r) ro[r + HALO] = a.sx * min(r, nr + HALO - 1);
    auto chunk = [](const T* q) { return *reinterpret_cast<const cvec_t*>(q); };

    // the tile's metrics, once
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    const T* mdx = static_cast<const T*>(p.dxfc) + m0;
    const T* mdy = static_cast<const T*>(p.dycf) + m0;
    const T* maf = static_cast<const T*>(p.azff) + m0;
    T dxfc[NR][W], dycf[NR][W + 1], azff[NR][W];                   // rows -3 .. JT + 2; -2 .. JT + 2, columns -1 .. W - 1; -2 .. JT + 2
    T dxcf[JT + 1][W + 1], dyfc[JT + 1][W + 1], azcc[JT + 1][W + 1];
    T azfc[JT][W], azcf[JT][W];
    int mu[JT][W], mv[JT][W];
    {
#pragma unroll
        for (int r = -HALO; r < JT + HALO; ++r) {
            const cvec_t x = chunk(mdx + ro[r + HALO]);
#pragma unroll
            for (int e = 0; e < W; ++e) dxfc[r + HALO][e] = x[e];
            if (r > -HALO) {
                const cvec_t y = chunk(mdy + ro[r + HALO]), f = chunk(maf + ro[r + HALO]);
                dycf[r + HALO][0] = mdy[ro[r + HALO] - 1];
#pragma unroll
                for (int e = 0; e < W; ++e) { dycf[r + HALO][e + 1] = y[e]; azff[r + HALO][e] = f[e]; }
            }
        }
        const T* px = static_cast<const T*>(p.dxcf) + m0;          // rows 0 .. JT, columns -1 .. W - 1
#pragma unroll
        for (int r = 0; r <= JT; ++r) {
            const cvec_t x = chunk(px + ro[r + HALO]);
            dxcf[r][0] = px[ro[r + HALO] - 1];
#pragma unroll
            for (int e = 0; e < W; ++e) dxcf[r][e + 1] = x[e];
        }
        const T* qy = static_cast<const T*>(p.dyfc) + m0;          // rows -1 .. JT - 1, columns 0 .. W
        if constexpr (FULL) {
            const T* ac = static_cast<const T*>(p.azcc) + m0;      // rows -1 .. JT - 1, columns -1 .. W - 1 (row -1: 0 .. W - 1)
#pragma unroll
            for (int r = -1; r < JT; ++r) {
                const cvec_t y = chunk(qy + ro[r + HALO]), c = chunk(ac + ro[r + HALO]);
                dyfc[r + 1][W] = qy[ro[r + HALO] + W];
                if (r >= 0) azcc[r + 1][0] = ac[ro[r + HALO] - 1];
#pragma unroll
                for (int e = 0; e < W; ++e) { dyfc[r + 1][e] = y[e]; azcc[r + 1][e + 1] = c[e]; }
            }
        } else {
#pragma unroll
            for (int r = -1; r < JT; ++r) {
                const cvec_t y = chunk(qy + ro[r + HALO]);
                dyfc[r + 1][W] = qy[ro[r + HALO] + W];
#pragma unroll
                for (int e = 0; e < W; ++e) dyfc[r + 1][e] = y[e];
            }
        }
        if constexpr (FULL) {
            const T* fu = static_cast<const T*>(p.azfc) + m0;
            const T* fv = static_cast<const T*>(p.azcf) + m0;
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                const cvec_t x = chunk(fu + ro[r + HALO]), y = chunk(fv + ro[r + HALO]);
#pragma unroll
                for (int e = 0; e < W; ++e) { azfc[r][e] = x[e]; azcf[r][e] = y[e]; mu[r][e] = 0; mv[r][e] = 0; }
                if constexpr (MASK) {                              // a count plane has no halo: clamped onto the last interior row
                    const long long n0 = (long long)a.Nx * (j0 + min(r, nr - 1)) + e0;
                    const Counts<W> nu = *reinterpret_cast<const Counts<W>*>(p.nfc + n0);
                    const Counts<W> nv = *reinterpret_cast<const Counts<W>*>(p.ncf + n0);
#pragma unroll
                    for (int e = 0; e < W; ++e) {                  // masked levels (0-based k < m)
                        mu[r][e] = min(max(nu[e], 0), a.Nz);
                        mv[r][e] = min(max(nv[e], 0), a.Nz);
                    }
                }
            }
        }
    }

    const long long f0 = a.off3 + (long long)a.sx * j0 + e0;
    const T* u = static_cast<const T*>(p.u) + f0;
    const T* v = static_cast<const T*>(p.v) + f0;
    const T* w = static_cast<const T*>(p.w) + f0;                  // face 1 of the tile's first cell; face k + 1 is one plane up per level
    const T* dz = static_cast<const T*>(p.dz);
    T* Gu = static_cast<T*>(p.Gu) + f0;
    T* Gv = static_cast<T*>(p.Gv) + f0;
    const T mval = (T)a.value;

    // w of one face: rows -1 .. JT - 1, columns -1 .. W - 1 (row -1: 0 .. W - 1)
    auto load_w = [&](T (&wf)[JT + 1][W + 1], const T* wk) {
#pragma unroll
        for (int r = -1; r < JT; ++r) {
            const cvec_t x = chunk(wk + ro[r + HALO]);
            if (r >= 0) wf[r + 1][0] = wk[ro[r + HALO] - 1];
#pragma unroll
            for (int e = 0; e < W; ++e) wf[r + 1][e + 1] = x[e];
        }
    };
    // the JT rows of the chunk of one plane
    auto load_rows = [&](T (&x)[JT][W], const T* q) {
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            const cvec_t c = chunk(q + ro[r + HALO]);
#pragma unroll
            for (int e = 0; e < W; ++e) x[r][e] = c[e];
        }
    };
    // S and R at one face: w there, u and v above and below it, dz_f there
    auto face_terms = [&](const T (&wf)[JT + 1][W + 1], const T (&uhi)[JT][W], const T (&ulo)[JT][W], const T (&vhi)[JT][W],
                          const T (&vlo)[JT][W], T d, T (&S)[JT][W], T (&R)[JT][W]) {
#pragma unroll
        for (int r = 0; r < JT; ++r)
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const T A = azcc[r + 1][e + 1] * wf[r + 1][e + 1];
                const T Aw = azcc[r + 1][e] * wf[r + 1][e];
                const T As = azcc[r][e + 1] * wf[r][e + 1];
                S[r][e] = (half * (Aw + A)) * ((uhi[r][e] - ulo[r][e]) / d);
                R[r][e] = (half * (As + A)) * ((vhi[r][e] - vlo[r][e]) / d);
            }
    };
    // Z at row r of the tile and column c of the chunk, any c in -2 .. W + 2, from element loads: the rule's operations, the same bits as the
    // Z a neighbouring item forms on its own columns.  Reads columns c - 1 .. c: e0 - 3 .. e0 + W + 2, inside the row (Hx >= 3)
    auto zeta_at = [&](const T* uk, const T* vk, int r, int c) -> T {
        const long long o = (long long)ro[r + HALO] + c, os = (long long)ro[r + HALO - 1] + c;
        return ((mdy[o] * vk[o] - mdy[o - 1] * vk[o - 1]) - (mdx[o] * uk[o] - mdx[os] * uk[os])) / maf[o];
    };
    // UB and VB (SW::VS) at the node of that Z, from the elements of u and v zeta_at reads there: the same bits as a neighbouring item's own
    auto ub_at = [&](const T* uk, int r, int c) -> T {
        const long long o = (long long)ro[r + HALO] + c, os = (long long)ro[r + HALO - 1] + c;
        return half * (uk[os] + uk[o]);
    };
    auto vb_at = [&](const T* vk, int r, int c) -> T {
        const long long o = (long long)ro[r + HALO] + c;
        return half * (vk[o - 1] + vk[o]);
    };

    struct Level {
        T u[NR][W + 2], v[NR][W + 2];                              // this level: the cells around the chunk's rows (FULL: those rows are carried)
        T wt[JT + 1][W + 1];                                       // w at the level's TOP face
        T ua[JT][W], va[JT][W];                                    // the chunk's rows one level up
        T d;                                                       // dz_f of the top face
    };
    auto load = [&](Level& L, int k) {                             // FULL
        const T* uk = u + a.plane * k;
        const T* vk = v + a.plane * k;
        L.d = dz[k + 1];
#pragma unroll
        for (int r = -HALO; r < JT + HALO; ++r) {
            if (r < 0 || r >= JT) {                                // the rows south and north of the tile on the chunk's columns
                const cvec_t x = chunk(uk + ro[r + HALO]);
#pragma unroll
                for (int e = 0; e < W; ++e) L.u[r + HALO][e + 1] = x[e];
                if (r > -HALO) {
                    const cvec_t y = chunk(vk + ro[r + HALO]);
#pragma unroll
                    for (int e = 0; e < W; ++e) L.v[r + HALO][e + 1] = y[e];
                }
            }
            if (r > -HALO) L.v[r + HALO][0] = vk[ro[r + HALO] - 1];             // v[i - 1, .]: rows -2 .. JT + 2
            if (r >= 0 && r < JT) L.u[r + HALO][0] = uk[ro[r + HALO] - 1];      // u[i - 1, .]: the tile's rows
            if (r >= -1 && r < JT) L.u[r + HALO][W + 1] = uk[ro[r + HALO] + W]; // u[i + 1, .]: rows -1 .. JT - 1
        }
        load_w(L.wt, w + a.plane * (k + 1));
        load_rows(L.ua, uk + a.plane);
        load_rows(L.va, vk + a.plane);
    };

    // carried from level to level: the chunk's u, v rows of the level and S, R at its bottom face (the top face of the level below)
    T uc[JT][W], vc[JT][W], Sb[JT][W], Rb[JT][W];
    if constexpr (FULL) {
        T w1[JT + 1][W + 1], u0[JT][W], v0[JT][W];
        load_w(w1, w);
        load_rows(uc, u);
        load_rows(vc, v);
        load_rows(u0, u - a.plane);                                // the bottom halo plane
        load_rows(v0, v - a.plane);
        face_terms(w1, uc, u0, vc, v0, dz[0], Sb, Rb);
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
            Level L;
            if constexpr (FULL) {
                if constexpr (LA == 0) load(ring[s], k);
                L = ring[s];
                if constexpr (LA > 0) { if (k + LA < a.Nz) load(ring[s], k + LA); }   // the loads of level k + LA go out before level k's arithmetic
            } else {
                // all rows of u (v: from -2) at the level itself, written here and not through `load`: through the lambda the compiler
                // forms every address before the first load, and the Float64 form was 1.2 % of the whole call slower for it
                // (profiles/vorticity_kernel/)
                static_assert(FULL || LA == 0, "the vorticity term alone is built without a ring");
                const T* uk = u + a.plane * k;
                const T* vk = v + a.plane * k;
#pragma unroll
                for (int r = -HALO; r < JT + HALO; ++r) {
                    const cvec_t x = chunk(uk + ro[r + HALO]);
#pragma unroll
                    for (int e = 0; e < W; ++e) L.u[r + HALO][e + 1] = x[e];
                    if (r > -HALO) {
                        const cvec_t y = chunk(vk + ro[r + HALO]);
#pragma unroll
                        for (int e = 0; e < W; ++e) L.v[r + HALO][e + 1] = y[e];
                        L.v[r + HALO][0] = vk[ro[r + HALO] - 1];                        // v[i - 1, .]: rows -2 .. JT + 2
                    }
                    if (r >= -1 && r < JT) L.u[r + HALO][W + 1] = uk[ro[r + HALO] + W]; // u[i + 1, .]: rows -1 .. JT - 1
                }
            }
            if constexpr (FULL) {
#pragma unroll
                for (int r = 0; r < JT; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) { L.u[r + HALO][e + 1] = uc[r][e]; L.v[r + HALO][e + 1] = vc[r][e]; }
            }
            T St[JT][W], Rt[JT][W];
            if constexpr (FULL) face_terms(L.wt, L.ua, uc, L.va, vc, L.d, St, Rt);
            // Z on the chunk's columns: rows -2 .. JT + 2, indexed [r + 2]
            T Z[JT + 5][W];
#pragma unroll
            for (int r = -2; r < JT + HALO; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e)
                    Z[r + 2][e] = ((dycf[r + HALO][e + 1] * L.v[r + HALO][e + 1] - dycf[r + HALO][e] * L.v[r + HALO][e])
                                   - (dxfc[r + HALO][e] * L.u[r + HALO][e + 1] - dxfc[r + HALO - 1][e] * L.u[r + HALO - 1][e + 1])) / azff[r + HALO][e];
            // Z of the tile's rows on the columns -2 .. W + 2, indexed [c + 2]: the chunk's own, two from the lane to the west, three from
            // the lane to the east (W = 2: two, and one from the lane after it) -- or, where that lane holds another chunk, formed here
            T zx[JT][W + 5];
            {
                const T* uk = u + a.plane * k;
                const T* vk = v + a.plane * k;
#pragma unroll
                for (int r = 0; r < JT; ++r) {
#pragma unroll
                    for (int e = 0; e < W; ++e) zx[r][e + 2] = Z[r + 2][e];
                    if constexpr (SW::SHARE) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) zx[r][q] = __shfl_up(Z[r + 2][W - 2 + q], 1);
#pragma unroll
                        for (int q = 0; q < 3; ++q) zx[r][W + 2 + q] = q < W ? __shfl_down(Z[r + 2][q % W], 1) : __shfl_down(Z[r + 2][q % W], 2);
                    }
                    if (!west_ok) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) zx[r][q] = zeta_at(uk, vk, r, q - 2);
                    }
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (!(q < W ? east1_ok : east2_ok)) zx[r][W + 2 + q] = zeta_at(uk, vk, r, W + q);
                }
            }
            // SW::VS: UB and VB at the nodes of Z, indexed as Z and zx are
            T UB[JT + 5][W], VB[JT + 5][W], ubx[JT][W + 5], vbx[JT][W + 5];
            if constexpr (SW::VS) {
                const T* uk = u + a.plane * k;
                const T* vk = v + a.plane * k;
#pragma unroll
                for (int r = -2; r < JT + HALO; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        UB[r + 2][e] = half * (L.u[r + HALO - 1][e + 1] + L.u[r + HALO][e + 1]);
                        VB[r + 2][e] = half * (L.v[r + HALO][e] + L.v[r + HALO][e + 1]);
                    }
#pragma unroll
                for (int r = 0; r < JT; ++r) {
#pragma unroll
                    for (int e = 0; e < W; ++e) { ubx[r][e + 2] = UB[r + 2][e]; vbx[r][e + 2] = VB[r + 2][e]; }
                    if constexpr (SW::SHARE_VS) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            ubx[r][q] = __shfl_up(UB[r + 2][W - 2 + q], 1);
                            vbx[r][q] = __shfl_up(VB[r + 2][W - 2 + q], 1);
                        }
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            ubx[r][W + 2 + q] = q < W ? __shfl_down(UB[r + 2][q % W], 1) : __shfl_down(UB[r + 2][q % W], 2);
                            vbx[r][W + 2 + q] = q < W ? __shfl_down(VB[r + 2][q % W], 1) : __shfl_down(VB[r + 2][q % W], 2);
                        }
                    }
                    if (!(SW::SHARE_VS && west_ok)) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) { ubx[r][q] = ub_at(uk, r, q - 2); vbx[r][q] = vb_at(vk, r, q - 2); }
                    }
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        if (!(SW::SHARE_VS && (q < W ? east1_ok : east2_ok))) { ubx[r][W + 2 + q] = ub_at(uk, r, W + q); vbx[r][W + 2 + q] = vb_at(vk, r, W + q); }
                }
            }
            // P: rows 0 .. JT, columns -1 .. W - 1.  Q: rows -1 .. JT - 1, columns 0 .. W.  K: rows -1 .. JT - 1, columns -1 .. W - 1, without (-1, -1)
            T P[JT + 1][W + 1], Q[JT + 1][W + 1], K[JT + 1][W + 1];
#pragma unroll
            for (int r = 0; r <= JT; ++r)
#pragma unroll
                for (int e = 0; e <= W; ++e) {
                    P[r][e] = dxcf[r][e] * L.v[r + HALO][e];
                    Q[r][e] = dyfc[r][e] * L.u[r + HALO - 1][e + 1];
                    if constexpr (FULL) {
                        if (r == 0 && e == 0) continue;
                        const T ua = L.u[r + HALO - 1][e], ub = L.u[r + HALO - 1][e + 1], va = L.v[r + HALO - 1][e], vb = L.v[r + HALO][e];
                        K[r][e] = half * (half * (ua * ua + ub * ub) + half * (va * va + vb * vb));
                    }
                }
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                cvec_t gu, gv;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    {
                        const T vh = half * (half * (P[r][e] + P[r + 1][e]) + half * (P[r][e + 1] + P[r + 1][e + 1]));
                        const T vhat = vh / dxfc[r + HALO][e];
                        const bool pos = vhat >= T(0);             // true for -0, false for NaN
                        T zr;
                        if constexpr (SW::VS)
                            zr = weno_face_vs<T>(pos ? Z[r][e] : Z[r + 5][e], pos ? Z[r + 1][e] : Z[r + 4][e], pos ? Z[r + 2][e] : Z[r + 3][e],
                                                 pos ? Z[r + 3][e] : Z[r + 2][e], pos ? Z[r + 4][e] : Z[r + 1][e],
                                                 pos ? UB[r][e] : UB[r + 5][e], pos ? UB[r + 1][e] : UB[r + 4][e], pos ? UB[r + 2][e] : UB[r + 3][e],
                                                 pos ? UB[r + 3][e] : UB[r + 2][e], pos ? UB[r + 4][e] : UB[r + 1][e],
                                                 pos ? VB[r][e] : VB[r + 5][e], pos ? VB[r + 1][e] : VB[r + 4][e], pos ? VB[r + 2][e] : VB[r + 3][e],
                                                 pos ? VB[r + 3][e] : VB[r + 2][e], pos ? VB[r + 4][e] : VB[r + 1][e]);
                        else
                            zr = weno_face<T>(pos ? Z[r][e] : Z[r + 5][e], pos ? Z[r + 1][e] : Z[r + 4][e], pos ? Z[r + 2][e] : Z[r + 3][e],
                                              pos ? Z[r + 3][e] : Z[r + 2][e], pos ? Z[r + 4][e] : Z[r + 1][e]);     // Z[r + 2 + m][e]: Z[i, j + m]
                        const T hu = -(vhat * zr);
                        if constexpr (FULL) {
                            const T bu = (K[r + 1][e + 1] - K[r + 1][e]) / dxfc[r + HALO][e];
                            const T vu = (half * (Sb[r][e] + St[r][e])) / azfc[r][e];
                            const T g = -((hu + vu) + bu);
                            gu[e] = (MASK && k < mu[r][e]) ? mval : g;
                        } else {
                            gu[e] = hu;
                        }
                    }
                    {
                        const T uh = half * (half * (Q[r][e] + Q[r][e + 1]) + half * (Q[r + 1][e] + Q[r + 1][e + 1]));
                        const T uhat = uh / dycf[r + HALO][e + 1];
                        const bool pos = uhat >= T(0);
                        T zr;
                        if constexpr (SW::VS)
                            zr = weno_face_vs<T>(pos ? zx[r][e] : zx[r][e + 5], pos ? zx[r][e + 1] : zx[r][e + 4], pos ? zx[r][e + 2] : zx[r][e + 3],
                                                 pos ? zx[r][e + 3] : zx[r][e + 2], pos ? zx[r][e + 4] : zx[r][e + 1],
                                                 pos ? ubx[r][e] : ubx[r][e + 5], pos ? ubx[r][e + 1] : ubx[r][e + 4], pos ? ubx[r][e + 2] : ubx[r][e + 3],
                                                 pos ? ubx[r][e + 3] : ubx[r][e + 2], pos ? ubx[r][e + 4] : ubx[r][e + 1],
                                                 pos ? vbx[r][e] : vbx[r][e + 5], pos ? vbx[r][e + 1] : vbx[r][e + 4], pos ? vbx[r][e + 2] : vbx[r][e + 3],
                                                 pos ? vbx[r][e + 3] : vbx[r][e + 2], pos ? vbx[r][e + 4] : vbx[r][e + 1]);
                        else
                            zr = weno_face<T>(pos ? zx[r][e] : zx[r][e + 5], pos ? zx[r][e + 1] : zx[r][e + 4], pos ? zx[r][e + 2] : zx[r][e + 3],
                                              pos ? zx[r][e + 3] : zx[r][e + 2], pos ? zx[r][e + 4] : zx[r][e + 1]);   // zx[r][e + 2 + m]: Z[i + m, j]
                        const T hv = uhat * zr;
                        if constexpr (FULL) {
                            const T bv = (K[r + 1][e + 1] - K[r][e + 1]) / dycf[r + HALO][e + 1];
                            const T vv = (half * (Rb[r][e] + Rt[r][e])) / azcf[r][e];
                            const T g = -((hv + vv) + bv);
                            gv[e] = (MASK && k < mv[r][e]) ? mval : g;
                        } else {
                            gv[e] = hv;
                        }
                    }
                }
                if (r < nr) {
                    store_chunk<SW::NT>(reinterpret_cast<cvec_t*>(Gu + a.plane * k + a.sx * r), gu);
                    store_chunk<SW::NT>(reinterpret_cast<cvec_t*>(Gv + a.plane * k + a.sx * r), gv);
                }
            }
            if constexpr (FULL) {
#pragma unroll
                for (int r = 0; r < JT; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) { uc[r][e] = L.ua[r][e]; vc[r][e] = L.va[r][e]; Sb[r][e] = St[r][e]; Rb[r][e] = Rt[r][e]; }
            }
        }
    }
}

}  // namespace
