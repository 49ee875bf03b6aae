// tpg_momentum.hip -- the vector-invariant advection tendency of the horizontal velocities, Gu at (Face, Center, Center) and Gv at
// (Center, Face, Center), for gfx950 (tpg_momentum_advection_tendency): what the AB2 step of the velocities (tpg_ab2_step_velocities)
// consumes as Gu, Gv.
// [recalled: Oceananigans' U_dot_grad_u / U_dot_grad_v for VectorInvariant() with EnstrophyConserving vorticity, the zeta2 w / zeta1 w vertical
// terms and the gradient of Kh at (Center, Center, Center); parity unpinned, like every operator here]
//
// The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with no
// contraction.  Every operation is one correctly rounded IEEE operation.  kf is a face index; w has Nz + 1 levels.
//     Z[i,j,k]  = ((dy_cf[i,j] v[i,j,k] - dy_cf[i-1,j] v[i-1,j,k]) - (dx_fc[i,j] u[i,j,k] - dx_fc[i,j-1] u[i,j-1,k])) / az_ff[i,j]
//     P[i,j,k]  = dx_cf[i,j] * v[i,j,k]      Q[i,j,k] = dy_fc[i,j] * u[i,j,k]      A[i,j,kf] = az_cc[i,j] * w[i,j,kf]
//     K[i,j,k]  = T(0.5) * (T(0.5) * (u[i,j,k]*u[i,j,k] + u[i+1,j,k]*u[i+1,j,k]) + T(0.5) * (v[i,j,k]*v[i,j,k] + v[i,j+1,k]*v[i,j+1,k]))
//  u: zb = T(0.5) * (Z[i,j,k] + Z[i,j+1,k])
//     vh = T(0.5) * (T(0.5) * (P[i-1,j,k] + P[i-1,j+1,k]) + T(0.5) * (P[i,j,k] + P[i,j+1,k]))
//     hu = -((zb * vh) / dx_fc[i,j])
//     bu = (K[i,j,k] - K[i-1,j,k]) / dx_fc[i,j]
//     S[i,j,kf] = (T(0.5) * (A[i-1,j,kf] + A[i,j,kf])) * ((u[i,j,kf] - u[i,j,kf-1]) / dz_f[kf])        kf = 1..Nz+1
//     vu = (T(0.5) * (S[i,j,k] + S[i,j,k+1])) / az_fc[i,j]
//     Gu[i,j,k] = -((hu + vu) + bu)
//  v: zb = T(0.5) * (Z[i,j,k] + Z[i+1,j,k])
//     uh = T(0.5) * (T(0.5) * (Q[i,j-1,k] + Q[i+1,j-1,k]) + T(0.5) * (Q[i,j,k] + Q[i+1,j,k]))
//     hv = (zb * uh) / dy_cf[i,j]
//     bv = (K[i,j,k] - K[i,j-1,k]) / dy_cf[i,j]
//     R[i,j,kf] = (T(0.5) * (A[i,j-1,kf] + A[i,j,kf])) * ((v[i,j,kf] - v[i,j,kf-1]) / dz_f[kf])
//     vv = (T(0.5) * (R[i,j,k] + R[i,j,k+1])) / az_cf[i,j]
//     Gv[i,j,k] = -((hv + vv) + bv)
// - Each of Z, P, Q, K, A, S, R has one definition: forming it once or again at a tile edge gives the same bits.  Leading minus signs are
//   sign flips.  A zero divisor divides, as the rule says.
// - Cells read, relative to the node: u at (0,0), (+-1,0), (0,+-1), (1,-1) and k+-1 at (0,0); v at (0,0), (+-1,0), (0,+-1), (-1,1) and
//   k+-1 at (0,0); w at faces k, k+1 at (0,0), (-1,0), (0,-1).  Corner halo cells are read.  So Hx, Hy, Hz >= 1, and the caller has filled
//   every halo of u and v and the horizontal halos of w.  Only interior cells of Gu, Gv are written.
// - Mask: with the count planes n_fc, n_cf, the nodes k <= min(max(n, 0), Nz) of Gu (by n_fc) and Gv (by n_cf) hold T(mask_value) instead;
//   everything is computed unmasked -- bit for bit what tpg_mask_immersed_fields leaves.
//
// ONE launch for both fields, of the family of k_tracer_advection (tpg_advection.hip) and k_w_from_continuity (tpg_continuity.hip): a work
// item is ONE chunk of W interior columns x JT rows and walks ALL levels innermost, so u, v and w are each fetched once for both
// tendencies.  The item loads once the cells of the eight metric planes its nodes read and the count values.  It carries from level to
// level S and R at the level's bottom face and the u, v rows of the level (which are "the level below" of the next): each plane is
// fetched once for the vertical direction.  Per level: dz_f of the top face (wave-uniform), the JT rows of u and v one level up, the row
// south and the row north of the tile and the elements west and east of each row of u and v at this level, and the JT rows of w at the top
// face with the row south and the elements west.  No load depends on the previous level: the loads of the next LOOKAHEAD levels are
// issued before the current level's arithmetic (a ring of register slots).  Items are numbered (row tile, chunk) with the chunk fastest,
// 256 to a block.  Rows of the last tile past the interior compute on the row offsets clamped onto row Ny + 1 (inside the north halo) and
// store nothing.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_momentum_tendency.hpp"
#include "../../include/tripolar_hip_momentum.h"

// compile-time switches of the A/B in profiles/momentum/ (make MOMENTUM_TAG=_jt2 MOMENTUM_FLAGS=-DTPG_MOM_JT=2, -DTPG_MOM_JT_F32=1,
// -DTPG_MOM_LOOKAHEAD=2, -DTPG_MOM_LOOKAHEAD_F32=1, -DTPG_MOM_NT=0 or -DTPG_MOM_WAVES=2).  What was measured at 3600 x 1800 x 75 and why
// these are the defaults: DESIGN.md 6, profiles/momentum/.
#ifndef TPG_MOM_JT
#define TPG_MOM_JT 1
#endif
#ifndef TPG_MOM_JT_F32
#define TPG_MOM_JT_F32 2
#endif
#ifndef TPG_MOM_LOOKAHEAD
#define TPG_MOM_LOOKAHEAD 1
#endif
#ifndef TPG_MOM_LOOKAHEAD_F32
#define TPG_MOM_LOOKAHEAD_F32 2
#endif
#ifndef TPG_MOM_NT
#define TPG_MOM_NT 1
#endif
#ifndef TPG_MOM_WAVES
#define TPG_MOM_WAVES 1
#endif

namespace {

template <typename T> constexpr int ROWS = sizeof(T) == 8 ? TPG_MOM_JT : TPG_MOM_JT_F32;                   // rows per work item (JT below)
template <typename T> constexpr int LOOKAHEAD = sizeof(T) == 8 ? TPG_MOM_LOOKAHEAD : TPG_MOM_LOOKAHEAD_F32;   // levels whose loads are in flight
constexpr bool NT = TPG_MOM_NT;            // Gu, Gv go out in streaming stores
constexpr int WAVES = TPG_MOM_WAVES;       // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)

// Arrays of the tile are indexed [r + 1][c + 1] where a row r = -1 or a column c = -1 is read, [r][c] otherwise: r = -1 is the row south
// of the tile, r = JT the row north of it, c = -1 the column west of the chunk, c = W the column east of it.  Entries the rule does not
// read are never loaded and never used.
template <typename T, int W, bool GEN, bool MASK, int JT, int LA>
__global__ __launch_bounds__(256, WAVES) void k_momentum_advection(MomentumPtrs p, MomentumArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int e0 = (item - tile * a.cpr) * W;                      // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const T half = T(0.5);

    // row offsets inside a plane, rows -1 .. JT of the tile: the rows past the interior clamped onto the row north of the last interior one
    // (row nr <= Ny of the tile: inside the interior or the first north halo row, Hy >= 1)
    int ro[JT + 2];
#pragma unroll
    for (int r = -1; r <= JT; ++r) ro[r + 1] = a.sx * min(r, nr);
    auto chunk = [](const T* q) { return *reinterpret_cast<const cvec_t*>(q); };

    // the tile's metrics, once
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    T dxfc[JT + 2][W + 1], dycf[JT + 1][W + 2], azff[JT + 1][W + 1], dxcf[JT + 1][W + 1], dyfc[JT + 1][W + 1], azcc[JT + 1][W + 1];
    T azfc[JT][W], azcf[JT][W];
    int mu[JT][W], mv[JT][W];
    {
        const T* dx = static_cast<const T*>(p.dxfc) + m0;          // rows -1 .. JT, columns 0 .. W (row JT: 0 .. W - 1)
#pragma unroll
        for (int r = -1; r <= JT; ++r) {
            const cvec_t x = chunk(dx + ro[r + 1]);
#pragma unroll
            for (int e = 0; e < W; ++e) dxfc[r + 1][e] = x[e];
            if (r < JT) dxfc[r + 1][W] = dx[ro[r + 1] + W];
        }
        const T* dy = static_cast<const T*>(p.dycf) + m0;          // rows 0 .. JT, columns -1 .. W (row JT: -1 .. W - 1)
        const T* af = static_cast<const T*>(p.azff) + m0;          // rows 0 .. JT, columns 0 .. W (row JT: 0 .. W - 1)
        const T* px = static_cast<const T*>(p.dxcf) + m0;          // rows 0 .. JT, columns -1 .. W - 1
#pragma unroll
        for (int r = 0; r <= JT; ++r) {
            const cvec_t y = chunk(dy + ro[r + 1]), f = chunk(af + ro[r + 1]), x = chunk(px + ro[r + 1]);
            dycf[r][0] = dy[ro[r + 1] - 1];
            dxcf[r][0] = px[ro[r + 1] - 1];
#pragma unroll
            for (int e = 0; e < W; ++e) { dycf[r][e + 1] = y[e]; azff[r][e] = f[e]; dxcf[r][e + 1] = x[e]; }
            if (r < JT) { dycf[r][W + 1] = dy[ro[r + 1] + W]; azff[r][W] = af[ro[r + 1] + W]; }
        }
        const T* qy = static_cast<const T*>(p.dyfc) + m0;          // rows -1 .. JT - 1, columns 0 .. W
        const T* ac = static_cast<const T*>(p.azcc) + m0;          // rows -1 .. JT - 1, columns -1 .. W - 1 (row -1: 0 .. W - 1)
#pragma unroll
        for (int r = -1; r < JT; ++r) {
            const cvec_t y = chunk(qy + ro[r + 1]), c = chunk(ac + ro[r + 1]);
            dyfc[r + 1][W] = qy[ro[r + 1] + W];
            if (r >= 0) azcc[r + 1][0] = ac[ro[r + 1] - 1];
#pragma unroll
            for (int e = 0; e < W; ++e) { dyfc[r + 1][e] = y[e]; azcc[r + 1][e + 1] = c[e]; }
        }
        const T* fu = static_cast<const T*>(p.azfc) + m0;
        const T* fv = static_cast<const T*>(p.azcf) + m0;
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            const cvec_t x = chunk(fu + ro[r + 1]), y = chunk(fv + ro[r + 1]);
#pragma unroll
            for (int e = 0; e < W; ++e) { azfc[r][e] = x[e]; azcf[r][e] = y[e]; mu[r][e] = 0; mv[r][e] = 0; }
            if constexpr (MASK) {                                  // a count plane has no halo: clamped onto the last interior row
                const long long n0 = (long long)a.Nx * (j0 + min(r, nr - 1)) + e0;
                const Counts<W> nu = *reinterpret_cast<const Counts<W>*>(p.nfc + n0);
                const Counts<W> nv = *reinterpret_cast<const Counts<W>*>(p.ncf + n0);
#pragma unroll
                for (int e = 0; e < W; ++e) {                      // masked levels (0-based k < m)
                    mu[r][e] = min(max(nu[e], 0), a.Nz);
                    mv[r][e] = min(max(nv[e], 0), a.Nz);
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
            const cvec_t x = chunk(wk + ro[r + 1]);
            if (r >= 0) wf[r + 1][0] = wk[ro[r + 1] - 1];
#pragma unroll
            for (int e = 0; e < W; ++e) wf[r + 1][e + 1] = x[e];
        }
    };
    // the JT rows of the chunk of one plane
    auto load_rows = [&](T (&x)[JT][W], const T* q) {
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            const cvec_t c = chunk(q + ro[r + 1]);
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

    struct Level {
        T u[JT + 2][W + 2], v[JT + 2][W + 2];                      // this level: the neighbours of the chunk's rows (those rows are carried)
        T wt[JT + 1][W + 1];                                       // w at the level's TOP face
        T ua[JT][W], va[JT][W];                                    // the chunk's rows one level up
        T d;                                                       // dz_f of the top face
    };
    auto load = [&](Level& L, int k) {
        const T* uk = u + a.plane * k;
        const T* vk = v + a.plane * k;
        L.d = dz[k + 1];
        const cvec_t us = chunk(uk + ro[0]), un = chunk(uk + ro[JT + 1]), vs = chunk(vk + ro[0]), vn = chunk(vk + ro[JT + 1]);
        L.u[0][W + 1] = uk[ro[0] + W];                             // u[i + 1, j - 1]: the south-east corner
        L.v[JT + 1][0] = vk[ro[JT + 1] - 1];                       // v[i - 1, j + 1]: the north-west corner
#pragma unroll
        for (int e = 0; e < W; ++e) { L.u[0][e + 1] = us[e]; L.u[JT + 1][e + 1] = un[e]; L.v[0][e + 1] = vs[e]; L.v[JT + 1][e + 1] = vn[e]; }
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            L.u[r + 1][0] = uk[ro[r + 1] - 1];
            L.u[r + 1][W + 1] = uk[ro[r + 1] + W];
            L.v[r + 1][0] = vk[ro[r + 1] - 1];
            L.v[r + 1][W + 1] = vk[ro[r + 1] + W];
        }
        load_w(L.wt, w + a.plane * (k + 1));
        load_rows(L.ua, uk + a.plane);
        load_rows(L.va, vk + a.plane);
    };

    // carried from level to level: the chunk's u, v rows of the level and S, R at its bottom face (the top face of the level below)
    T uc[JT][W], vc[JT][W], Sb[JT][W], Rb[JT][W];
    {
        T w1[JT + 1][W + 1], u0[JT][W], v0[JT][W];
        load_w(w1, w);
        load_rows(uc, u);
        load_rows(vc, v);
        load_rows(u0, u - a.plane);                                // the bottom halo plane
        load_rows(v0, v - a.plane);
        face_terms(w1, uc, u0, vc, v0, dz[0], Sb, Rb);
    }

    Level ring[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) load(ring[s], min(s, a.Nz - 1));
    for (int k0 = 0; k0 < a.Nz; k0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int k = k0 + s;
            if (k >= a.Nz) break;
            Level L = ring[s];
            if (k + LA < a.Nz) load(ring[s], k + LA);              // the loads of level k + LA go out before level k's arithmetic
#pragma unroll
            for (int r = 0; r < JT; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e) { L.u[r + 1][e + 1] = uc[r][e]; L.v[r + 1][e + 1] = vc[r][e]; }
            T St[JT][W], Rt[JT][W];
            face_terms(L.wt, L.ua, uc, L.va, vc, L.d, St, Rt);
            // Z: rows 0 .. JT, columns 0 .. W, without (JT, W)
            T Z[JT + 1][W + 1];
#pragma unroll
            for (int r = 0; r <= JT; ++r)
#pragma unroll
                for (int e = 0; e <= W; ++e) {
                    if (r == JT && e == W) continue;
                    Z[r][e] = ((dycf[r][e + 1] * L.v[r + 1][e + 1] - dycf[r][e] * L.v[r + 1][e])
                               - (dxfc[r + 1][e] * L.u[r + 1][e + 1] - dxfc[r][e] * L.u[r][e + 1])) / azff[r][e];
                }
            // P: rows 0 .. JT, columns -1 .. W - 1.  Q: rows -1 .. JT - 1, columns 0 .. W.  K: rows -1 .. JT - 1, columns -1 .. W - 1, without (-1, -1)
            T P[JT + 1][W + 1], Q[JT + 1][W + 1], K[JT + 1][W + 1];
#pragma unroll
            for (int r = 0; r <= JT; ++r)
#pragma unroll
                for (int e = 0; e <= W; ++e) {
                    P[r][e] = dxcf[r][e] * L.v[r + 1][e];
                    Q[r][e] = dyfc[r][e] * L.u[r][e + 1];
                    if (r == 0 && e == 0) continue;
                    const T ua = L.u[r][e], ub = L.u[r][e + 1], va = L.v[r][e], vb = L.v[r + 1][e];
                    K[r][e] = half * (half * (ua * ua + ub * ub) + half * (va * va + vb * vb));
                }
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                cvec_t gu, gv;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    {
                        const T zb = half * (Z[r][e] + Z[r + 1][e]);
                        const T vh = half * (half * (P[r][e] + P[r + 1][e]) + half * (P[r][e + 1] + P[r + 1][e + 1]));
                        const T hu = -((zb * vh) / dxfc[r + 1][e]);
                        const T bu = (K[r + 1][e + 1] - K[r + 1][e]) / dxfc[r + 1][e];
                        const T vu = (half * (Sb[r][e] + St[r][e])) / azfc[r][e];
                        const T g = -((hu + vu) + bu);
                        gu[e] = (MASK && k < mu[r][e]) ? mval : g;
                    }
                    {
                        const T zb = half * (Z[r][e] + Z[r][e + 1]);
                        const T uh = half * (half * (Q[r][e] + Q[r][e + 1]) + half * (Q[r + 1][e] + Q[r + 1][e + 1]));
                        const T hv = (zb * uh) / dycf[r][e + 1];
                        const T bv = (K[r + 1][e + 1] - K[r][e + 1]) / dycf[r][e + 1];
                        const T vv = (half * (Rb[r][e] + Rt[r][e])) / azcf[r][e];
                        const T g = -((hv + vv) + bv);
                        gv[e] = (MASK && k < mv[r][e]) ? mval : g;
                    }
                }
                if (r < nr) {
                    store_chunk<NT>(reinterpret_cast<cvec_t*>(Gu + a.plane * k + a.sx * r), gu);
                    store_chunk<NT>(reinterpret_cast<cvec_t*>(Gv + a.plane * k + a.sx * r), gv);
                }
            }
#pragma unroll
            for (int r = 0; r < JT; ++r)
#pragma unroll
                for (int e = 0; e < W; ++e) { uc[r][e] = L.ua[r][e]; vc[r][e] = L.va[r][e]; Sb[r][e] = St[r][e]; Rb[r][e] = Rt[r][e]; }
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_momentum_last_error(void) { return tpg_last_error(); }

int tpg_momentum_advection_tendency(const void* u, const void* v, const void* w, void* Gu, void* Gv, const void* dx_fc, const void* dy_fc,
                                    const void* az_fc, const void* dx_cf, const void* dy_cf, const void* az_cf, const void* az_cc,
                                    const void* az_ff, const void* dz_f, const int32_t* n_fc, const int32_t* n_cf, double mask_value, int scheme,
                                    int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (scheme != TPG_MOMENTUM_ENSTROPHY_CONSERVING) {
        tpg::set_error("momentum advection scheme %d is not built (TPG_MOMENTUM_ENSTROPHY_CONSERVING = 0 is)", scheme);
        return TPG_ERR_UNSUPPORTED;
    }
    const MomentumCall call{ u, v, w, Gu, Gv, dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_f, n_fc, n_cf, mask_value,
                             tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft };
    if (int rc = call.check(1, "u, v[i-1..i+1, j-1..j+1, k-1..k+1] and w[i-1, j], w[i, j-1]")) return rc;
    return call.launch(ROWS<double>, ROWS<float>, "k_momentum_advection", stream, [](auto ty, auto cw, auto gen, auto mask) {
        typedef decltype(ty) T;
        return k_momentum_advection<T, decltype(cw)::value, decltype(gen)::value, decltype(mask)::value, ROWS<T>, LOOKAHEAD<T>>;
    });
}

}  // extern "C"
