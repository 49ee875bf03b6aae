// tpg_continuity.hip -- the horizontal divergence at (Center, Center, Center) and w at (Center, Center, Face) from continuity, for gfx950
// (tpg_w_from_continuity).
//
// What a hydrostatic model runs after every velocity update, before its time-step wizard and its output writer read model.velocities:
// the continuity equation integrated upward from the bottom.  [recalled: Oceananigans' `div_xyᶜᶜᶜ` and `_compute_w_from_continuity!`; parity
// unpinned, like every operator here.]
//
// Fields
// - `u` at (Face, Center, Center) and `v` at (Center, Face, Center): padded parents of geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
// - `w` at (Center, Center, Face): a padded parent with `Nz + 1` interior levels, `Nz + 1 + 2Hz` planes, same `sx`, `sy`.
// - `div` at (Center, Center, Center): a parent like u's.
// Metrics
// - The grid's padded planes `dy_fc` (`Δyᶠᶜᵃ`), `dx_cf` (`Δxᶜᶠᵃ`), `az_cc` (`Azᶜᶜᵃ`), halos built.
// - `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]` in the field type.
// Arithmetic, for every interior column `i = 1..Nx`, `j = 1..Ny`, in the field type, in exactly this order, no contraction, every operation
// one correctly rounded IEEE operation:
//     w[i,j,1] = +0
//     for k = 1..Nz, d = dz_c[k]:
//         fe = (dy_fc[i+1,j] * d) * u[i+1,j,k]        fw = (dy_fc[i,j] * d) * u[i,j,k]
//         fn = (dx_cf[i,j+1] * d) * v[i,j+1,k]        fs = (dx_cf[i,j] * d) * v[i,j,k]
//         V  = az_cc[i,j] * d
//         div[i,j,k] = (1 / V) * ((fe - fw) + (fn - fs))
//         w[i,j,k+1] = w[i,j,k] - d * div[i,j,k]
// - `fe` of column `i` IS `fw` of column `i+1`. `fn` of row `j` IS `fs` of row `j+1`. Each is formed once.
// - Cells read: `u[1..Nx+1, 1..Ny, 1..Nz]` and the same cells of `dy_fc`; `v[1..Nx, 1..Ny+1, 1..Nz]` and the same cells of `dx_cf`;
//   `az_cc` interior; `dz_c`.
// - That is one halo column to the east and one halo row to the north, so `Hx ≥ 1` and `Hy ≥ 1`. The caller has filled the halos of u and v.
// - On a latitude band `Ny` is the band's row count and row `Ny+1` the exchanged (or, on the last band, folded) north halo row.
// - Only interior cells of `w` (levels `1..Nz+1`) and `div` are written.
// - `V = 0` divides by it, as the rule says.
//
// HBM-bound, of the family of k_vertical_vorticity (tpg_operators.hip): two streams read, one (w) or two (w and div) written, metrics in
// registers, levels innermost.  It differs in one respect: the vertical scan is a recurrence in k, so a work item is ONE chunk of W interior
// columns x JT rows x ALL levels -- level segments would re-associate the sum, which is not the rule.  The item loads once dy_fc of the chunk
// and its east neighbour, dx_cf of rows j0 .. j0+JT, az_cc, the count values, and keeps the running w (JT x W values).  Per level: d from
// dz_c[k] (wave-uniform), JT rows of u plus the east neighbour element (the same or the next cache line), JT + 1 rows of v, the shared
// fluxes formed once, one streaming vector store per row of w and / or div.  Only `w - d * div` depends on the previous level; no load does:
// the loads of the next LOOKAHEAD levels are issued before the current level's arithmetic (a ring of register slots), which is the one
// thing that would otherwise serialise on HBM latency.  Items are numbered (row tile, chunk) with the chunk fastest, 256 to a block.
// Rows of the last tile past the interior compute on the clamped last row and store nothing.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  No atomics, no LDS, nothing allocated, no host wait.
//
// Fused mask (n_cc given): the scan runs on the unmasked values (levels under the mask ARE read: a model's u and v are masked there); where
// they are stored, div nodes k <= n and w faces k <= min(n + 1, Nz) get `mask_value` (converted once to T) instead -- bit for bit what
// tpg_mask_immersed_fields leaves on w (TPG_FACE) and div (TPG_CENTER) with that plane.
#include "tpg_operator.hpp"
#include "../../include/tripolar_hip_continuity.h"

// compile-time switches of the A/B in profiles/continuity/ (make CONTINUITY_FLAGS='-DTPG_CONT_JT=4 -DTPG_CONT_LOOKAHEAD=1' or -DTPG_CONT_NT=0)
#ifndef TPG_CONT_JT
#define TPG_CONT_JT 4
#endif
#ifndef TPG_CONT_LOOKAHEAD
#define TPG_CONT_LOOKAHEAD 2
#endif
#ifndef TPG_CONT_NT
#define TPG_CONT_NT 1
#endif

namespace {

constexpr int JT = TPG_CONT_JT;            // rows per work item
constexpr int LA = TPG_CONT_LOOKAHEAD;     // levels whose loads are in flight ahead of the arithmetic
constexpr bool NT = TPG_CONT_NT;          // w and div go out in streaming stores

struct ContPtrs {
    const void *u, *v;
    void *w, *div;
    const void *dy, *dx, *az, *dz;
    const int32_t* ncc;
};

struct ContArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int items;                             // row tiles x cpr
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double value;                          // the mask value (a T value held in a double)
};

template <typename T, int W, bool GEN, bool MASK, bool HAS_W, bool HAS_DIV>
__global__ __launch_bounds__(256) void k_w_from_continuity(ContPtrs p, ContArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int e0 = (item - tile * a.cpr) * W;                      // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior

    // row offsets inside a plane: the tile's rows (clamped onto its last interior row) and, for v and dx_cf, the row to the north of each
    int ro[JT + 1];
#pragma unroll
    for (int r = 0; r <= JT; ++r) ro[r] = a.sx * min(r, nr);
    int uo[JT];
#pragma unroll
    for (int r = 0; r < JT; ++r) uo[r] = a.sx * min(r, nr - 1);

    // the tile's metrics, once
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    const T* dy = static_cast<const T*>(p.dy) + m0;
    const T* dx = static_cast<const T*>(p.dx) + m0;
    const T* az = static_cast<const T*>(p.az) + m0;
    T dyc[JT][W + 1], dxr[JT + 1][W], azr[JT][W], wr[JT][W];
    int m[JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t y = *reinterpret_cast<const cvec_t*>(dy + uo[r]);
        const cvec_t z = *reinterpret_cast<const cvec_t*>(az + uo[r]);
        dyc[r][W] = dy[uo[r] + W];                                 // dy_fc[i + 1, j] of the chunk's last column
#pragma unroll
        for (int e = 0; e < W; ++e) { dyc[r][e] = y[e]; azr[r][e] = z[e]; wr[r][e] = T(0); m[r][e] = 0; }
        if constexpr (MASK) {
            const Counts<W> n = *reinterpret_cast<const Counts<W>*>(p.ncc + (long long)a.Nx * (j0 + min(r, nr - 1)) + e0);
#pragma unroll
            for (int e = 0; e < W; ++e) m[r][e] = min(n[e], a.Nz);  // masked div levels (0-based k < m); w faces f < min(m + 1, Nz)
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
    const T* dz = static_cast<const T*>(p.dz);
    T* w = HAS_W ? static_cast<T*>(p.w) + f0 : nullptr;
    T* div = HAS_DIV ? static_cast<T*>(p.div) + f0 : nullptr;
    const T mv = (T)a.value;

    struct Level {
        cvec_t u[JT], v[JT + 1];
        T ue[JT], d;
    };
    auto load = [&](Level& L, int k) {
        const T* uk = u + a.plane * k;
        const T* vk = v + a.plane * k;
        L.d = dz[k];
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            L.u[r] = *reinterpret_cast<const cvec_t*>(uk + uo[r]);
            L.ue[r] = uk[uo[r] + W];                               // u[i + 1, j, k] of the chunk's last column
        }
#pragma unroll
        for (int r = 0; r <= JT; ++r) L.v[r] = *reinterpret_cast<const cvec_t*>(vk + ro[r]);
    };

    if constexpr (HAS_W) {                                         // face 1: +0, masked wherever a plane is given with n >= 0
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            cvec_t out;
#pragma unroll
            for (int e = 0; e < W; ++e) out[e] = (MASK && 0 < min(m[r][e] + 1, a.Nz)) ? mv : T(0);
            if (r < nr) store_chunk<NT>(reinterpret_cast<cvec_t*>(w + a.sx * r), out);
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
            T fs[W];                                               // (dx_cf[i, j] * d) * v[i, j, k]: the previous row's fn
#pragma unroll
            for (int e = 0; e < W; ++e) fs[e] = (dxr[0][e] * d) * L.v[0][e];
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                T ux[W + 1];
#pragma unroll
                for (int e = 0; e < W; ++e) ux[e] = L.u[r][e];
                ux[W] = L.ue[r];
                T fw = (dyc[r][0] * d) * ux[0];                    // for e > 0 it is the fe of e - 1
                cvec_t dout, wout;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const T fe = (dyc[r][e + 1] * d) * ux[e + 1];
                    const T fn = (dxr[r + 1][e] * d) * L.v[r + 1][e];
                    const T V = azr[r][e] * d;
                    const T dv = (T(1) / V) * ((fe - fw) + (fn - fs[e]));
                    fw = fe;
                    fs[e] = fn;
                    dout[e] = (MASK && k < m[r][e]) ? mv : dv;
                    if constexpr (HAS_W) {
                        wr[r][e] = wr[r][e] - d * dv;
                        wout[e] = (MASK && k < m[r][e] && k + 1 < a.Nz) ? mv : wr[r][e];
                    }
                }
                if (r < nr) {
                    const long long o = a.plane * k + a.sx * r;
                    if constexpr (HAS_DIV) store_chunk<NT>(reinterpret_cast<cvec_t*>(div + o), dout);
                    if constexpr (HAS_W) store_chunk<NT>(reinterpret_cast<cvec_t*>(w + o + a.plane), wout);
                }
            }
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_continuity_last_error(void) { return tpg_last_error(); }

int tpg_w_from_continuity(const void* u, const void* v, void* w, void* div, const void* dy_fc, const void* dx_cf, const void* az_cc,
                          const void* dz_c, const int32_t* n_cc, double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft,
                          void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (!u || !v) { tpg::set_error("null u or v"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!w && !div) { tpg::set_error("w and div both null: nothing to compute"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!dy_fc || !dx_cf || !az_cc || !dz_c) { tpg::set_error("null dy_fc, dx_cf, az_cc or dz_c"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    if (misaligned(esz, u, v, w, div)) {
        tpg::set_error("u, v, w or div pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (misaligned(esz, dy_fc, dx_cf, az_cc, dz_c)) {
        tpg::set_error("dy_fc, dx_cf, az_cc or dz_c pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if ((uintptr_t)n_cc % 4) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz;            // u, v, div
    const unsigned long long wbytes = (unsigned long long)g.plane * (Nz + 1 + 2 * Hz) * esz;       // w: one more level
    if (w && (arrays_overlap(w, wbytes, u, bytes) || arrays_overlap(w, wbytes, v, bytes))) {
        tpg::set_error("w's parent overlaps u's or v's (every column reads cells while its neighbours' columns write)");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (div && (arrays_overlap(div, bytes, u, bytes) || arrays_overlap(div, bytes, v, bytes))) {
        tpg::set_error("div's parent overlaps u's or v's (every column reads cells while its neighbours' columns write)");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (w && div && arrays_overlap(w, wbytes, div, bytes)) { tpg::set_error("w's parent overlaps div's"); return TPG_ERR_INVALID_ARGUMENT; }
    if (Hx < 1 || Hy < 1) {
        tpg::set_error("the rule reads u[i+1, j] and v[i, j+1]: Hx >= 1 and Hy >= 1 needed (halo (%d,%d))", Hx, Hy);
        return TPG_ERR_UNSUPPORTED;
    }
    const long long tiles = (Ny + JT - 1) / JT;
    if (tiles * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("continuity: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    const ContPtrs p{ u, v, w, div, dy_fc, dx_cf, az_cc, dz_c, n_cc };
    hipStream_t st = tpg::as_stream(stream);
    void* arrays[7] = { const_cast<void*>(u), const_cast<void*>(v), const_cast<void*>(dy_fc), const_cast<void*>(dx_cf), const_cast<void*>(az_cc) };
    int na = 5;
    if (w) arrays[na++] = w;
    if (div) arrays[na++] = div;
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        const ContArgs a{ Nx, Ny, Nz, g.sx, cpr, (int)(tiles * cpr), g.plane, interior2(g), interior3(g), n_cc ? (double)(T)mask_value : 0.0 };
        dim3 grid((unsigned)((a.items + 255) / 256));
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto outputs = [&](auto mask) {
                constexpr bool MASK = decltype(mask)::value;
                if (w && div)  hipLaunchKernelGGL((k_w_from_continuity<T, W, GEN, MASK, true, true>), grid, dim3(256), 0, st, p, a);
                else if (w)    hipLaunchKernelGGL((k_w_from_continuity<T, W, GEN, MASK, true, false>), grid, dim3(256), 0, st, p, a);
                else           hipLaunchKernelGGL((k_w_from_continuity<T, W, GEN, MASK, false, true>), grid, dim3(256), 0, st, p, a);
            };
            if (n_cc) outputs(std::true_type{});
            else      outputs(std::false_type{});
        });
        return tpg::launch_status("k_w_from_continuity");
    });
}

}  // extern "C"
