// tpg_weno_vi_finish_kernel.hpp -- the ONE kernel that finishes a momentum tendency upwinded in every term, the second launch of
// tpg_weno_vi_momentum_advection_tendency (tpg_weno_vi.hip) and of tpg_weno_vs_momentum_advection_tendency (tpg_weno_vs.hip): it reads hu, hv
// back from Gu, Gv at its own nodes, forms the upwinded vertical term and the upwinded kinetic-energy gradient of
// include/tripolar_hip_weno_vi.h and stores -((hu + vu) + bu), -((hv + vvert) + bv), masked.  Which smoothness stencil formed hu and hv
// (the first launch: tpg_weno_vorticity_kernel.hpp) does not enter it.  The including file passes NT (Gu, Gv go out in streaming stores)
// as the last template argument.  The description of the kernel is in tpg_weno_vi.hip, where it was written.
#pragma once
#include "tpg_momentum_tendency.hpp"
#include "tpg_weno_face.hpp"
#include "tpg_weno_vorticity_kernel.hpp"

namespace {

constexpr int WIN = 5;                     // levels of the z-window carried from level to level

// ---- launch 2: the upwinded vertical term and kinetic-energy gradient, and the last line ---------------------------------------------------------
template <typename T>
__device__ __forceinline__ T c4(T a, T b, T c, T d) { return (T(7) / T(12)) * (b + c) - (T(1) / T(12)) * (a + d); }

// vel >= 0 ? W5F(q[0..4]; s[0..4]) : W5F(q[5..1]; s[5..1]) for the six values at -3 .. +2 of the face: ten selects, one W5F
template <typename T>
__device__ __forceinline__ T upwind_fs(T vel, const T (&q)[6], const T (&s)[6])
{
    const bool pos = vel >= T(0);                                  // true for -0, false for NaN
    return weno_face_fs<T>(pos ? q[0] : q[5], pos ? q[1] : q[4], pos ? q[2] : q[3], pos ? q[3] : q[2], pos ? q[4] : q[1],
                           pos ? s[0] : s[5], pos ? s[1] : s[4], pos ? s[2] : s[3], pos ? s[3] : s[2], pos ? s[4] : s[1]);
}

// ZF of the header for the six levels x0 .. x5 = f - 3 .. f + 2 around face f (between x2 and x3) of class `cls`, which is the same in
// every lane: the inputs are selected, the face value is evaluated once
template <typename T>
__device__ __forceinline__ T z_face(int cls, T M, T x0, T x1, T x2, T x3, T x4, T x5)
{
    const bool pos = M >= T(0);
    if (cls == WENO_Z_ORDER5) return weno_face<T>(pos ? x0 : x5, pos ? x1 : x4, pos ? x2 : x3, pos ? x3 : x2, pos ? x4 : x1);
    if (cls == WENO_Z_ORDER3) return weno_face3<T>(pos ? x1 : x4, pos ? x2 : x3, pos ? x3 : x2);
    if (cls == WENO_Z_ORDER1) return pos ? x2 : x3;
    return T(0.5) * (x2 + x3);
}

// Rows are r = -3 .. +3 around the item's row, columns c = -3 .. W + 2 around its chunk (c = 0 .. W - 1 the chunk's).
template <typename T, int W, bool GEN, bool MASK, bool NT>
__global__ __launch_bounds__(256, 1) void k_weno_vi_finish(MomentumPtrs p, MomentumArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int j0 = item / a.cpr;                                   // the item's interior row (0-based): one row per item
    const int ch = item - j0 * a.cpr;
    const int e0 = ch * W;                                         // first interior column of the chunk (0-based)
    const T half = T(0.5);
    int ro[2 * HALO + 1];                                          // rows -3 .. +3: j0 - 3 >= -3 and j0 + 3 <= Ny + 2 lie inside the halos (Hy >= 3)
#pragma unroll
    for (int r = -HALO; r <= HALO; ++r) ro[r + HALO] = a.sx * r;
    auto chunk = [](const T* q) { return *reinterpret_cast<const cvec_t*>(q); };

    // the item's metrics, once.  Row arrays are indexed [c + 3] (az: [c + 2]), column arrays [r + 3] (az: [r + 2])
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    T dyr[W + 6], dyy[6][W + 1];                                   // dy_fc: row 0, columns -3 .. W + 2; rows -3 .. +2, columns 0 .. W
    T dxr[2][W + 5], dxy[7][W];                                    // dx_cf: rows 0, 1, columns -3 .. W + 1; rows -3 .. +3, the chunk's columns
    T azr[W + 3], azy[4][W];                                       // az_cc: row 0, columns -2 .. W; rows -2 .. +1, the chunk's columns
    T dxfc[W], dycf[W], azfc[W], azcf[W];
    int mu[W], mv[W];
    {
        const T* my = static_cast<const T*>(p.dyfc) + m0;
        const T* mx = static_cast<const T*>(p.dxcf) + m0;
        const T* mz = static_cast<const T*>(p.azcc) + m0;
#pragma unroll
        for (int r = -HALO; r < HALO; ++r) {
            const cvec_t y = chunk(my + ro[r + HALO]);
#pragma unroll
            for (int e = 0; e < W; ++e) dyy[r + HALO][e] = y[e];
            dyy[r + HALO][W] = my[ro[r + HALO] + W];
        }
#pragma unroll
        for (int c = -HALO; c < W + HALO; ++c) dyr[c + HALO] = (c >= 0 && c <= W) ? dyy[HALO][c] : my[c];
#pragma unroll
        for (int r = -HALO; r <= HALO; ++r) {
            const cvec_t x = chunk(mx + ro[r + HALO]);
#pragma unroll
            for (int e = 0; e < W; ++e) dxy[r + HALO][e] = x[e];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = -HALO; c < W + 2; ++c) dxr[r][c + HALO] = (c >= 0 && c < W) ? dxy[r + HALO][c] : mx[ro[r + HALO] + c];
#pragma unroll
        for (int r = -2; r < 2; ++r) {
            const cvec_t z = chunk(mz + ro[r + HALO]);
#pragma unroll
            for (int e = 0; e < W; ++e) azy[r + 2][e] = z[e];
        }
#pragma unroll
        for (int c = -2; c <= W; ++c) azr[c + 2] = (c >= 0 && c < W) ? azy[2][c] : mz[c];
        const cvec_t x = chunk(static_cast<const T*>(p.dxfc) + m0), y = chunk(static_cast<const T*>(p.dycf) + m0);
        const cvec_t fu = chunk(static_cast<const T*>(p.azfc) + m0), fv = chunk(static_cast<const T*>(p.azcf) + m0);
#pragma unroll
        for (int e = 0; e < W; ++e) { dxfc[e] = x[e]; dycf[e] = y[e]; azfc[e] = fu[e]; azcf[e] = fv[e]; mu[e] = 0; mv[e] = 0; }
        if constexpr (MASK) {                                      // a count plane has no halo
            const long long n0 = (long long)a.Nx * j0 + e0;
            const Counts<W> nu = *reinterpret_cast<const Counts<W>*>(p.nfc + n0);
            const Counts<W> nv = *reinterpret_cast<const Counts<W>*>(p.ncf + n0);
#pragma unroll
            for (int e = 0; e < W; ++e) {                          // masked levels (0-based k < m)
                mu[e] = min(max(nu[e], 0), a.Nz);
                mv[e] = min(max(nv[e], 0), a.Nz);
            }
        }
    }

    const long long f0 = a.off3 + (long long)a.sx * j0 + e0;
    const T* u = static_cast<const T*>(p.u) + f0;                  // level 1 of the chunk; level L is min(L - 1, Nz) planes up (L <= Nz + 1)
    const T* v = static_cast<const T*>(p.v) + f0;
    const T* w = static_cast<const T*>(p.w) + f0;                  // face 1 of the chunk; face k + 1 is one plane up per level
    const T* dz = static_cast<const T*>(p.dz);
    T* Gu = static_cast<T*>(p.Gu) + f0;
    T* Gv = static_cast<T*>(p.Gv) + f0;
    const T mval = (T)a.value;

    // Wu and Wv at one face: A at row 0 on the columns -2 .. W and at the rows -2 .. +1 on the chunk's columns
    auto face_w = [&](const T* wk, T (&Wu)[W], T (&Wv)[W]) {
        T ay[4][W], ar[W + 3];
#pragma unroll
        for (int r = -2; r < 2; ++r) {
            const cvec_t x = chunk(wk + ro[r + HALO]);
#pragma unroll
            for (int e = 0; e < W; ++e) ay[r + 2][e] = azy[r + 2][e] * x[e];
        }
#pragma unroll
        for (int c = -2; c <= W; ++c) ar[c + 2] = (c >= 0 && c < W) ? ay[2][c] : azr[c + 2] * wk[c];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            Wu[e] = c4<T>(ar[e], ar[e + 1], ar[e + 2], ar[e + 3]);           // ar[e + 2 + m]: A[i + m, j]
            Wv[e] = c4<T>(ay[0][e], ay[1][e], ay[2][e], ay[3][e]);           // ay[2 + m][e]: A[i, j + m]
        }
    };

    // carried from level to level: the z-windows (win[s]: level K - 2 + s of the chunk, K the level, 1-based; the slots below level 1 hold
    // level 1 and are never selected) and FZu, FZv at the level's bottom face (the top face of the level below)
    T uw[WIN][W], vw[WIN][W], fzu[W], fzv[W];
    {
        T Wu[W], Wv[W];
        face_w(w, Wu, Wv);
        const cvec_t u0 = chunk(u - a.plane), u1 = chunk(u), u2 = chunk(u + a.plane * min(1, a.Nz)), u3 = chunk(u + a.plane * min(2, a.Nz));
        const cvec_t v0 = chunk(v - a.plane), v1 = chunk(v), v2 = chunk(v + a.plane * min(1, a.Nz)), v3 = chunk(v + a.plane * min(2, a.Nz));
#pragma unroll
        for (int e = 0; e < W; ++e) {
            uw[0][e] = u1[e]; uw[1][e] = u1[e]; uw[2][e] = u1[e]; uw[3][e] = u2[e]; uw[4][e] = u3[e];
            vw[0][e] = v1[e]; vw[1][e] = v1[e]; vw[2][e] = v1[e]; vw[3][e] = v2[e]; vw[4][e] = v3[e];
            fzu[e] = Wu[e] * (half * (u0[e] + u1[e]));             // face 1: the centred mean with the bottom halo plane
            fzv[e] = Wv[e] * (half * (v0[e] + v1[e]));
        }
    }

    for (int k = 0; k < a.Nz; ++k) {
        const T* uk = u + a.plane * k;
        const T* vk = v + a.plane * k;
        const T d = dz[k];
        // the level's loads.  The chunk's own cells of u and v are the windows' (uw[2], vw[2])
        const cvec_t hu = chunk(Gu + a.plane * k), hv = chunk(Gv + a.plane * k);
        const cvec_t un = chunk(u + a.plane * min(k + 3, a.Nz)), vn = chunk(v + a.plane * min(k + 3, a.Nz));    // level K + 3, clamped onto plane Nz + 1
        T ur[W + 6], uy[6][W + 1], ux[2];                          // u: row 0, columns -3 .. W + 2; rows -3 .. +2, columns 0 .. W; (-1, -1) and (W + 1, -1)
        T vr[2][W + 5], vy[7][W], vx[2];                           // v: rows 0, 1, columns -3 .. W + 1; rows -3 .. +3, the chunk's; (-1, -1) and (-1, 2)
#pragma unroll
        for (int c = -HALO; c < W + HALO; ++c) ur[c + HALO] = (c >= 0 && c < W) ? uw[2][c] : uk[c];
#pragma unroll
        for (int r = -HALO; r < HALO; ++r) {
            if (r == 0) {
#pragma unroll
                for (int e = 0; e <= W; ++e) uy[HALO][e] = ur[e + HALO];
            } else {
                const cvec_t x = chunk(uk + ro[r + HALO]);
#pragma unroll
                for (int e = 0; e < W; ++e) uy[r + HALO][e] = x[e];
                uy[r + HALO][W] = uk[ro[r + HALO] + W];
            }
        }
        ux[0] = uk[ro[HALO - 1] - 1];
        ux[1] = uk[ro[HALO - 1] + W + 1];
#pragma unroll
        for (int r = -HALO; r <= HALO; ++r) {
            if (r == 0) {
#pragma unroll
                for (int e = 0; e < W; ++e) vy[HALO][e] = vw[2][e];
            } else {
                const cvec_t x = chunk(vk + ro[r + HALO]);
#pragma unroll
                for (int e = 0; e < W; ++e) vy[r + HALO][e] = x[e];
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = -HALO; c < W + 2; ++c) vr[r][c + HALO] = (c >= 0 && c < W) ? vy[r + HALO][c] : vk[ro[r + HALO] + c];
        vx[0] = vk[ro[HALO - 1] - 1];
        vx[1] = vk[ro[HALO + 2] - 1];
        T Wu[W], Wv[W];
        face_w(w + a.plane * (k + 1), Wu, Wv);

        // FZu, FZv at the level's top face, face k + 2 (1-based): its class is the level's, the same in every lane
        const int cls = weno_z_face_class(k + 2, a.Nz);
        T fzut[W], fzvt[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            fzut[e] = Wu[e] * z_face<T>(cls, Wu[e], uw[0][e], uw[1][e], uw[2][e], uw[3][e], uw[4][e], un[e]);
            fzvt[e] = Wv[e] * z_face<T>(cls, Wv[e], vw[0][e], vw[1][e], vw[2][e], vw[3][e], vw[4][e], vn[e]);
        }

        // ---- u: everything along row 0, indexed [c + 3] ----
        cvec_t gu, gv;
        {
            T FX[W + 6], DU[W + 5], DV[W + 5], DS[W + 5], HU[W + 6], DKU[W + 5], SU[W + 5];
#pragma unroll
            for (int n = 0; n < W + 6; ++n) { FX[n] = (dyr[n] * ur[n]) * d; HU[n] = half * (ur[n] * ur[n]); }
#pragma unroll
            for (int n = 0; n < W + 5; ++n) {
                DU[n] = FX[n + 1] - FX[n];
                DV[n] = (dxr[1][n] * vr[1][n]) * d - (dxr[0][n] * vr[0][n]) * d;
                DS[n] = DU[n] + DV[n];
                DKU[n] = HU[n + 1] - HU[n];
                SU[n] = half * (ur[n] + ur[n + 1]);
            }
            // HV at the rows -1 .. +2 on the columns -1 .. W - 1, indexed [r + 1][c + 1]
            T HV[4][W + 1];
#pragma unroll
            for (int e = 0; e <= W; ++e) {
                const T a0 = e == 0 ? vx[0] : vy[HALO - 1][e - 1], a1 = vr[0][e + 2], a2 = vr[1][e + 2], a3 = e == 0 ? vx[1] : vy[HALO + 2][e - 1];
                HV[0][e] = half * (a0 * a0); HV[1][e] = half * (a1 * a1); HV[2][e] = half * (a2 * a2); HV[3][e] = half * (a3 * a3);
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const T uu = uw[2][e];
                const T dvs = c4<T>(DV[e + 1], DV[e + 2], DV[e + 3], DV[e + 4]);           // DV[e + 3 + m]: DV[i + m, j]
                const T q[6] = { DU[e], DU[e + 1], DU[e + 2], DU[e + 3], DU[e + 4], DU[e + 5] };      // DU[i - 3 .. i + 2, j]
                const T s[6] = { DS[e], DS[e + 1], DS[e + 2], DS[e + 3], DS[e + 4], DS[e + 5] };
                const T dur = upwind_fs<T>(uu, q, s);
                const T vu = (uu * (dvs + dur) + (fzut[e] - fzu[e])) / (azfc[e] * d);
                const T kus = c4<T>(HV[0][e + 1] - HV[0][e], HV[1][e + 1] - HV[1][e], HV[2][e + 1] - HV[2][e], HV[3][e + 1] - HV[3][e]);   // XKV[i, j - 1 .. j + 2]
                const T kq[6] = { DKU[e], DKU[e + 1], DKU[e + 2], DKU[e + 3], DKU[e + 4], DKU[e + 5] };
                const T ks[6] = { SU[e], SU[e + 1], SU[e + 2], SU[e + 3], SU[e + 4], SU[e + 5] };
                const T kur = upwind_fs<T>(uu, kq, ks);
                const T bu = (kur + kus) / dxfc[e];
                const T g = -((hu[e] + vu) + bu);
                gu[e] = (MASK && k < mu[e]) ? mval : g;
            }
        }
        // ---- v: everything along the chunk's columns, indexed [r + 3] ----
        {
            // HU at the rows -1, 0 on the columns -1 .. W + 1, indexed [c + 1]
            T HUs[W + 3], HUc[W + 3];
#pragma unroll
            for (int c = -1; c <= W + 1; ++c) {
                const T b = c < 0 ? ux[0] : (c > W ? ux[1] : uy[HALO - 1][c]), t = ur[c + HALO];
                HUs[c + 1] = half * (b * b);
                HUc[c + 1] = half * (t * t);
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const T vv = vw[2][e];
                T FY[7], HV[7], DU[6], DV[6], DS[6], DKV[6], SV[6];
#pragma unroll
                for (int r = 0; r < 7; ++r) { FY[r] = (dxy[r][e] * vy[r][e]) * d; HV[r] = half * (vy[r][e] * vy[r][e]); }
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    DU[r] = (dyy[r][e + 1] * uy[r][e + 1]) * d - (dyy[r][e] * uy[r][e]) * d;
                    DV[r] = FY[r + 1] - FY[r];
                    DS[r] = DU[r] + DV[r];
                    DKV[r] = HV[r + 1] - HV[r];
                    SV[r] = half * (vy[r][e] + vy[r + 1][e]);
                }
                const T dus = c4<T>(DU[1], DU[2], DU[3], DU[4]);                           // DU[3 + m]: DU[i, j + m]
                const T dvr = upwind_fs<T>(vv, DV, DS);
                const T vvert = (vv * (dus + dvr) + (fzvt[e] - fzv[e])) / (azcf[e] * d);
                const T kvs = c4<T>(HUc[e] - HUs[e], HUc[e + 1] - HUs[e + 1], HUc[e + 2] - HUs[e + 2], HUc[e + 3] - HUs[e + 3]);   // XKU[i - 1 .. i + 2, j]
                const T kvr = upwind_fs<T>(vv, DKV, SV);
                const T bv = (kvr + kvs) / dycf[e];
                const T g = -((hv[e] + vvert) + bv);
                gv[e] = (MASK && k < mv[e]) ? mval : g;
            }
        }
        store_chunk<NT>(reinterpret_cast<cvec_t*>(Gu + a.plane * k), gu);
        store_chunk<NT>(reinterpret_cast<cvec_t*>(Gv + a.plane * k), gv);
        // the windows and the faces move one level up
#pragma unroll
        for (int e = 0; e < W; ++e) {
#pragma unroll
            for (int s = 0; s + 1 < WIN; ++s) { uw[s][e] = uw[s + 1][e]; vw[s][e] = vw[s + 1][e]; }
            uw[WIN - 1][e] = un[e];
            vw[WIN - 1][e] = vn[e];
            fzu[e] = fzut[e];
            fzv[e] = fzvt[e];
        }
    }
}

}  // namespace
