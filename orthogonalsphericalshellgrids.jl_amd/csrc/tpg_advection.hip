// tpg_advection.hip -- the flux-form advection tendency of the tracers at (Center, Center, Center), for gfx950
// (tpg_tracer_advection_tendency): what the AB2 step of the tracers (tpg_ab2_step_fields) consumes as Gn.
// [recalled: Oceananigans' div_Uc with Centered(order = 2) in all three directions, _advective_tracer_flux_x/y/z, and
// hydrostatic_free_surface_tracer_tendency with no diffusion and no forcing; parity unpinned, like every operator here]
//
// The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with no
// contraction.  Every operation is one correctly rounded IEEE operation.
//     d = dz_c[k]
//     Mx[i,j,k] = (dy_fc[i,j] * d) * u[i,j,k]           i = 1..Nx+1     (the continuity's fe / fw, the same bits)
//     My[i,j,k] = (dx_cf[i,j] * d) * v[i,j,k]           j = 1..Ny+1
//     Mz[i,j,k] =  az_cc[i,j]      * w[i,j,k]           k = 1..Nz+1     (w has Nz+1 levels)
//     Fx[i,j,k] = Mx[i,j,k] * (T(0.5) * (c[i-1,j,k] + c[i,j,k]))
//     Fy[i,j,k] = My[i,j,k] * (T(0.5) * (c[i,j-1,k] + c[i,j,k]))
//     Fz[i,j,k] = Mz[i,j,k] * (T(0.5) * (c[i,j,k-1] + c[i,j,k]))
//     V = az_cc[i,j] * d
//     G[i,j,k] = -((T(1) / V) * (((Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])) + (Fz[i,j,k+1] - Fz[i,j,k])))
// - Each flux is formed once: Fx[i+1] of a column is Fx[i] of the next, Fz[k+1] of a level is Fz[k] of the next.  Recomputing one at a tile
//   edge gives the same bits.  The leading minus is a sign flip.  V = 0 divides by it, as the rule says.
// - Cells read: c[0..Nx+1, j, k], c[i, 0..Ny+1, k], c[i, j, 0..Nz+1] (a plus-shaped stencil, no corner halo cell); u[1..Nx+1, j, k],
//   v[i, 1..Ny+1, k], w[i, j, 1..Nz+1]; the same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.  So Hx, Hy, Hz >= 1, and the caller
//   has filled every halo of c, u and v.  Only interior cells of G are written.
// - Mask: with a (Center, Center) count plane n_cc, the nodes k <= min(max(n, 0), Nz) of G hold T(mask_value) instead; everything is
//   computed unmasked -- bit for bit what tpg_mask_immersed_fields leaves on a Center field.
// - Up to TPG_MAX_FIELDS tracers share one call; Mx, My, Mz do not depend on the tracer, so the results are bit-identical whether tracers
//   are computed together or one by one.
//
// HBM-bound, of the family of k_w_from_continuity (tpg_continuity.hip): a work item is ONE chunk of W interior columns x JT rows and walks
// ALL levels innermost, for TG tracers that share Mx, My, Mz and 1 / V (grid.y counts the tracer groups).  A call splits its tracers
// greedily into groups of 4, then of 2, then single ones (up to TPG_ADV_TG), one launch per group size, so a lone tracer pays nothing for a
// group's registers.  The item loads once dy_fc of the chunk and its east neighbour,
// dx_cf of rows j0 .. j0+JT, az_cc and the count values.  It carries from level to level, per tracer, Fz at the level's top face and the c
// rows of the level (which are "the level below" of the next): each c plane is fetched once for the vertical direction.  Per level: d from
// dz_c[k] (wave-uniform), JT rows of u plus the east neighbour element, JT + 1 rows of v, JT rows of w at the top face, and per tracer the JT
// rows of c one level up, the row south and the row north of the tile and one element west and east of each row at this level.  No load
// depends on the previous level: the loads of the next LOOKAHEAD levels are issued before the current level's arithmetic (a ring of register
// slots).  Items are numbered (row tile, chunk) with the chunk fastest, 256 to a block.  Rows of the last tile past the interior compute on
// the row offsets clamped onto row Ny + 1 (inside the north halo) and store nothing.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "tpg_tracer_tendency.hpp"
#include "../../include/tripolar_hip_advection.h"

// compile-time switches of the A/B in profiles/advection/ (make ADVECTION_TAG=_tg2 ADVECTION_FLAGS='-DTPG_ADV_TG=2', -DTPG_ADV_JT=4,
// -DTPG_ADV_LOOKAHEAD=1, -DTPG_ADV_LOOKAHEAD_F32=2, -DTPG_ADV_LOOKAHEAD_4=2, -DTPG_ADV_NT=0 or -DTPG_ADV_WAVES=2).  What was measured at
// 3600 x 1800 x 75 and why these are the defaults: DESIGN.md 6, profiles/advection/.
#ifndef TPG_ADV_TG
#define TPG_ADV_TG 4
#endif
#ifndef TPG_ADV_JT
#define TPG_ADV_JT 2
#endif
#ifndef TPG_ADV_LOOKAHEAD
#define TPG_ADV_LOOKAHEAD 2
#endif
#ifndef TPG_ADV_LOOKAHEAD_F32
#define TPG_ADV_LOOKAHEAD_F32 1
#endif
#ifndef TPG_ADV_LOOKAHEAD_4
#define TPG_ADV_LOOKAHEAD_4 1
#endif
#ifndef TPG_ADV_NT
#define TPG_ADV_NT 1
#endif
#ifndef TPG_ADV_WAVES
#define TPG_ADV_WAVES 1
#endif

namespace {

constexpr int GROUP = TPG_ADV_TG;          // the largest group of tracers a work item takes, sharing Mx, My, Mz: 4, 2 or 1 (no grouped kernel)
constexpr int JT = TPG_ADV_JT;             // rows per work item
// levels whose loads are in flight ahead of the arithmetic: groups of 4; one or two tracers in Float64 and in Float32
template <typename T, int TG> constexpr int LOOKAHEAD = TG >= 4 ? TPG_ADV_LOOKAHEAD_4 : sizeof(T) == 8 ? TPG_ADV_LOOKAHEAD : TPG_ADV_LOOKAHEAD_F32;
constexpr bool NT = TPG_ADV_NT;            // G goes out in streaming stores
constexpr int WAVES = TPG_ADV_WAVES;       // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)

struct AdvArgs {
    int Nx, Ny, Nz, sx;
    int q0;                                // the launch's first tracer
    int cpr;                               // chunks per interior row
    int items;                             // row tiles x cpr
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double value;                          // the mask value (a T value held in a double)
};

template <typename T, int W, bool GEN, bool MASK, int TG, int LA>
__global__ __launch_bounds__(256, WAVES) void k_tracer_advection(TracerPtrs p, AdvArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int e0 = (item - tile * a.cpr) * W;                      // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const int q0 = a.q0 + blockIdx.y * TG;                         // first tracer of the group

    // row offsets inside a plane: the tile's rows and the row to the north of the last, clamped onto the row north of the last interior one
    // (row nr <= Ny of the tile: inside the interior or the first north halo row, Hy >= 1)
    int ro[JT + 1];
#pragma unroll
    for (int r = 0; r <= JT; ++r) ro[r] = a.sx * min(r, nr);

    // the tile's metrics, once
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    const T* dy = static_cast<const T*>(p.dy) + m0;
    const T* dx = static_cast<const T*>(p.dx) + m0;
    const T* az = static_cast<const T*>(p.az) + m0;
    T dyc[JT][W + 1], dxr[JT + 1][W], azr[JT][W];
    int m[JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t y = *reinterpret_cast<const cvec_t*>(dy + ro[r]);
        const cvec_t z = *reinterpret_cast<const cvec_t*>(az + ro[r]);
        dyc[r][W] = dy[ro[r] + W];                                 // dy_fc[i + 1, j] of the chunk's last column
#pragma unroll
        for (int e = 0; e < W; ++e) { dyc[r][e] = y[e]; azr[r][e] = z[e]; m[r][e] = 0; }
        if constexpr (MASK) {                                      // a count plane has no halo: clamped onto the last interior row
            const Counts<W> n = *reinterpret_cast<const Counts<W>*>(p.ncc + (long long)a.Nx * (j0 + min(r, nr - 1)) + e0);
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

    struct Level {
        cvec_t u[JT], v[JT + 1], w[JT];                            // w at the level's TOP face
        T ue[JT], d;
        cvec_t ca[TG][JT], cs[TG], cn[TG];                         // c one level up; the rows south and north of the tile at this level
        T cw[TG][JT], ce[TG][JT];                                  // c one element west and east of each row at this level
    };
    auto load = [&](Level& L, int k) {
        const T* uk = u + a.plane * k;
        const T* vk = v + a.plane * k;
        const T* wk = w + a.plane * (k + 1);
        L.d = dz[k];
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            L.u[r] = *reinterpret_cast<const cvec_t*>(uk + ro[r]);
            L.ue[r] = uk[ro[r] + W];                               // u[i + 1, j, k] of the chunk's last column
            L.w[r] = *reinterpret_cast<const cvec_t*>(wk + ro[r]);
        }
#pragma unroll
        for (int r = 0; r <= JT; ++r) L.v[r] = *reinterpret_cast<const cvec_t*>(vk + ro[r]);
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            const T* ck = c[t] + a.plane * k;
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                L.ca[t][r] = *reinterpret_cast<const cvec_t*>(ck + a.plane + ro[r]);
                L.cw[t][r] = ck[ro[r] - 1];
                L.ce[t][r] = ck[ro[r] + W];
            }
            L.cs[t] = *reinterpret_cast<const cvec_t*>(ck - a.sx);
            L.cn[t] = *reinterpret_cast<const cvec_t*>(ck + ro[JT]);
        }
    };

    // carried from level to level: the c rows of the level and Fz at its bottom face (the top face of the level below)
    T cc[TG][JT][W], fzb[TG][JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t w1 = *reinterpret_cast<const cvec_t*>(w + ro[r]);
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            const cvec_t c1 = *reinterpret_cast<const cvec_t*>(c[t] + ro[r]);
            const cvec_t c0 = *reinterpret_cast<const cvec_t*>(c[t] - a.plane + ro[r]);      // the bottom halo plane
#pragma unroll
            for (int e = 0; e < W; ++e) {
                cc[t][r][e] = c1[e];
                fzb[t][r][e] = (azr[r][e] * w1[e]) * (T(0.5) * (c0[e] + c1[e]));
            }
        }
    }

    Level ring[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) load(ring[s], min(s, a.Nz - 1));
    for (int k0 = 0; k0 < a.Nz; k0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int k = k0 + s;
            if (k >= a.Nz) break;
            const Level L = ring[s];
            if (k + LA < a.Nz) load(ring[s], k + LA);              // the loads of level k + LA go out before level k's arithmetic
            const T d = L.d;
            T my[W];                                               // My at the south face of the row: the previous row's north face
            T fys[TG][W];                                          // Fy there, per tracer
#pragma unroll
            for (int e = 0; e < W; ++e) {
                my[e] = (dxr[0][e] * d) * L.v[0][e];
#pragma unroll
                for (int t = 0; t < TG; ++t) fys[t][e] = my[e] * (T(0.5) * (L.cs[t][e] + cc[t][0][e]));
            }
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                T mx[W + 1], mz[W], rV[W];
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    mx[e] = (dyc[r][e] * d) * L.u[r][e];
                    my[e] = (dxr[r + 1][e] * d) * L.v[r + 1][e];
                    mz[e] = azr[r][e] * L.w[r][e];
                    rV[e] = T(1) / (azr[r][e] * d);
                }
                mx[W] = (dyc[r][W] * d) * L.ue[r];
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    T cx[W + 2], cnr[W];                           // the row with its west and east neighbours; the row to the north
                    cx[0] = L.cw[t][r];
                    cx[W + 1] = L.ce[t][r];
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        cx[e + 1] = cc[t][r][e];
                        if (r + 1 < JT) cnr[e] = cc[t][(r + 1) % JT][e];
                        else cnr[e] = L.cn[t][e];
                    }
                    T fw = mx[0] * (T(0.5) * (cx[0] + cx[1]));     // for e > 0 it is the fe of e - 1
                    cvec_t out;
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const T fe = mx[e + 1] * (T(0.5) * (cx[e + 1] + cx[e + 2]));
                        const T fn = my[e] * (T(0.5) * (cx[e + 1] + cnr[e]));
                        const T fzt = mz[e] * (T(0.5) * (cx[e + 1] + L.ca[t][r][e]));
                        const T g = -(rV[e] * (((fe - fw) + (fn - fys[t][e])) + (fzt - fzb[t][r][e])));
                        fw = fe;
                        fys[t][e] = fn;
                        fzb[t][r][e] = fzt;
                        out[e] = (MASK && k < m[r][e]) ? mv : g;
                    }
                    if (r < nr) store_chunk<NT>(reinterpret_cast<cvec_t*>(G[t] + a.plane * k + a.sx * r), out);
                }
            }
#pragma unroll
            for (int t = 0; t < TG; ++t)
#pragma unroll
                for (int r = 0; r < JT; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) cc[t][r][e] = L.ca[t][r][e];
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_advection_last_error(void) { return tpg_last_error(); }

int tpg_tracer_advection_tendency(const void* const* c, void* const* G, int nfields, const void* u, const void* v, const void* w,
                                  const void* dy_fc, const void* dx_cf, const void* az_cc, const void* dz_c, const int32_t* n_cc,
                                  double mask_value, int scheme, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (scheme != TPG_ADVECTION_CENTERED2) {
        tpg::set_error("advection scheme %d is not built (TPG_ADVECTION_CENTERED2 = 0 is)", scheme);
        return TPG_ERR_UNSUPPORTED;
    }
    const TracerCall call{ c, G, nfields, u, v, w, dy_fc, dx_cf, az_cc, dz_c, n_cc, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft };
    if (int rc = call.check(1, 1, "c[i-1..i+1, j-1..j+1, k-1..k+1]")) return rc;
    const Geom& g = call.g;
    const long long tiles = (Ny + JT - 1) / JT;
    if (tiles * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("tracer advection: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    const TracerPtrs p = call.pointers();
    void* arrays[2 * TPG_MAX_FIELDS + 6];
    const int na = call.arrays(arrays);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        AdvArgs a{ Nx, Ny, Nz, g.sx, 0, cpr, (int)(tiles * cpr), g.plane, interior2(g), interior3(g), n_cc ? (double)(T)mask_value : 0.0 };
        const unsigned blocks = (unsigned)((a.items + 255) / 256);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto launch = [&](auto mask) {
                constexpr bool MASK = decltype(mask)::value;
                tracer_groups<GROUP>(nfields, [&](auto tg, int q0, int n) {
                    constexpr int TG = decltype(tg)::value;
                    a.q0 = q0;
                    hipLaunchKernelGGL((k_tracer_advection<T, W, GEN, MASK, TG, LOOKAHEAD<T, TG>>), dim3(blocks, n), dim3(256), 0, st, p, a);
                });
            };
            if (n_cc) launch(std::true_type{});
            else      launch(std::false_type{});
        });
        return tpg::launch_status("k_tracer_advection");
    });
}

}  // extern "C"
