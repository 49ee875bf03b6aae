// tpg_free_surface.hip -- one forward-backward sub-step of a split-explicit free surface (eta, U, V), for gfx950 (tpg_free_surface_substep):
// what runs `substeps` times between tpg_barotropic_mode and tpg_barotropic_correction (tpg_barotropic.hip).
// [recalled: Oceananigans' `_split_explicit_free_surface!` then `_split_explicit_barotropic_velocity!` on the new eta, ForwardBackwardScheme;
// parity unpinned, like every operator here.]
//
// Arrays
// - eta at (Center, Center), U, GU at (Face, Center), V, GV at (Center, Face), the averages, and the five metric planes dy_fc, dx_cf, az_cc,
//   dx_fc, dy_cf: 2-D padded planes of ONE geometry `(Ny + 2 Hy2) x (Nx + 2 Hx)`, row pitch `sx`, first interior cell `sx Hy2 + Hx`.
// - `depth_of_count`: `Nz + 1` values in the field type; `n_fc`, `n_cf`: null, or Ny x Nx int32 count planes.
// The rule, in the field type, in exactly this order, no contraction, every operation one correctly rounded IEEE operation:
//     fe = dy_fc[i+1,j] * U[i+1,j]      fw = dy_fc[i,j] * U[i,j]      fn = dx_cf[i,j+1] * V[i,j+1]      fs = dx_cf[i,j] * V[i,j]
//     eta'[i,j] = eta[i,j] - dtau * (((fe - fw) + (fn - fs)) / az_cc[i,j])
//     U'[i,j] = U[i,j] + dtau * (GU[i,j] - (g * Hfc) * ((eta'[i,j] - eta'[i-1,j]) / dx_fc[i,j]))          eta'[0,j] = eta'[Nx,j]
//     V'[i,j] = V[i,j] + dtau * (GV[i,j] - (g * Hcf) * ((eta'[i,j] - eta'[i,j-1]) / dy_cf[i,j]))          j >= 2;  V'[i,1] = V[i,1]
//     eta_bar += weight * eta',  U_bar += weight * U',  V_bar += weight * V'                              (optional, in place)
// with Hfc = depth_of_count[n_fc[i,j]], Hcf = depth_of_count[n_cf[i,j]] (counts clamped to 0..Nz; no plane: depth_of_count[0]).
// - Cells read beyond the interiors: column Nx+1 of U and dy_fc, row Ny+1 of V and dx_cf.  Only interior cells are written.
//
// ONE launch.  HBM-bound on large grids (about twenty planes move), launch-bound on small ones.  A work item is one chunk of W interior
// columns x JT rows, of the family of k_w_from_continuity: it sweeps its rows from the south, one row further south first, so that eta' of
// the row below is in registers when a row's V' is formed, and forms eta' of the column to its west alongside (for the first chunk of a row
// that is column Nx, whose east flux is the halo column's, as its owner forms it).  The products dy_fc * U and dx_cf * V are each formed once
// per item and shared by the cells on both sides: the same product, the same bits.  The redundant row and column come from L2 (the items
// that own them run beside this one); they cost (1 + 1/JT)(1 + 1/W) of stage 1's arithmetic, no HBM read.  Items are numbered (row tile,
// chunk) with the chunk fastest, 256 to a block.  Rows of the last tile past the interior compute on clamped rows and store nothing.
//
// eta, U, V ping-pong: an item reads only the `_in` arrays and writes only the `_out` ones, so no item reads a cell another writes.
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the planes passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "../../include/tripolar_hip_free_surface.h"

// compile-time switch of the A/B in profiles/free_surface/ (make FREE_SURFACE_TAG=_jt4 FREE_SURFACE_FLAGS=-DTPG_FS_JT=4).  Measured at
// 3600 x 1800, Hy2 = 31, averaging on: 2 rows per item are 2 % (Float64) and 4 - 5 % (Float32) faster than 4, 8 rows 8 - 10 % slower than 4:
// the extra row of stage 1 comes from L2 and costs less than the occupancy the longer items give up (98 - 178 VGPRs at 4 rows).
#ifndef TPG_FS_JT
#define TPG_FS_JT 2
#endif

namespace {

constexpr int JT = TPG_FS_JT;              // rows per work item

struct FsPtrs {
    void *eta_out, *U_out, *V_out;
    const void *eta, *U, *V, *GU, *GV;
    void *eta_bar, *U_bar, *V_bar;
    const void *dy_fc, *dx_cf, *az_cc, *dx_fc, *dy_cf, *depth;
    const int32_t *nfc, *ncf;
};

struct FsArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int items;                             // row tiles x cpr
    long long off2;                        // sx * Hy2 + Hx: the first interior cell of a plane
    double dtau, g, weight;                // T values held in doubles
};

template <typename T, int W, bool GEN, bool COUNTS, bool AVG>
__global__ __launch_bounds__(256) void k_free_surface_substep(FsPtrs p, FsArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int e0 = (item - tile * a.cpr) * W;                      // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const int cw = e0 ? e0 - 1 : a.Nx - 1;                         // the column to the west (0-based): the wrap for the first chunk
    const T dtau = (T)a.dtau, g = (T)a.g, wt = (T)a.weight;

    const T* U = static_cast<const T*>(p.U) + a.off2;              // [sx * j + i], j and i 0-based interior indices
    const T* V = static_cast<const T*>(p.V) + a.off2;
    const T* eta = static_cast<const T*>(p.eta) + a.off2;
    const T* dy = static_cast<const T*>(p.dy_fc) + a.off2;
    const T* dx = static_cast<const T*>(p.dx_cf) + a.off2;
    const T* az = static_cast<const T*>(p.az_cc) + a.off2;
    auto chunk = [&](const T* base, long long row) { return *reinterpret_cast<const cvec_t*>(base + row + e0); };

    // dx_cf * V of rows js = max(j0 - 1, 0) (slot 0) and j0 .. j0 + JT (slots 1 .. JT + 1, clamped onto row j0 + nr <= Ny, the north halo
    // row), own columns and the west column; the V rows themselves are kept for stage 2
    const long long rs = (long long)a.sx * max(j0 - 1, 0);
    T yf[JT + 2][W], yfw[JT + 2], Vr[JT][W];
    {
        const cvec_t v = chunk(V, rs), x = chunk(dx, rs);
#pragma unroll
        for (int e = 0; e < W; ++e) yf[0][e] = x[e] * v[e];
        yfw[0] = T(0);
    }
#pragma unroll
    for (int k = 1; k <= JT + 1; ++k) {
        const long long row = (long long)a.sx * (j0 + min(k - 1, nr));
        const cvec_t v = chunk(V, row), x = chunk(dx, row);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            yf[k][e] = x[e] * v[e];
            if (k <= JT) Vr[k - 1][e] = v[e];
        }
        yfw[k] = dx[row + cw] * V[row + cw];
    }

    // eta' of one row at the chunk's columns (and, WEST, at the column to the west): the x fluxes of the row formed once
    T Ur[W];                                                       // U of the row last swept, for stage 2
    auto sweep = [&](long long row, const T (&fs)[W], const T (&fn)[W], T fsw, T fnw, T (&etap)[W], T& ew, bool west) {
        const cvec_t u = chunk(U, row), y = chunk(dy, row), h = chunk(eta, row), z = chunk(az, row);
        T xf[W + 1];
#pragma unroll
        for (int e = 0; e < W; ++e) { xf[e] = y[e] * u[e]; Ur[e] = u[e]; }
        xf[W] = dy[row + e0 + W] * U[row + e0 + W];                // column i + 1 of the chunk's last column: the east halo column at the row's end
#pragma unroll
        for (int e = 0; e < W; ++e) etap[e] = h[e] - dtau * (((xf[e + 1] - xf[e]) + (fn[e] - fs[e])) / z[e]);
        if (west) {
            T few = xf[0];                                         // the west column's east flux: the chunk's first ...
            if (e0 == 0) few = dy[row + a.Nx] * U[row + a.Nx];     // ... or, for column Nx, the east halo column's, as its owner forms it
            const T fww = dy[row + cw] * U[row + cw];
            ew = eta[row + cw] - dtau * (((few - fww) + (fnw - fsw)) / az[row + cw]);
        }
    };

    T etas[W], etaw = T(0);
    sweep(rs, yf[0], yf[1], T(0), T(0), etas, etaw, false);        // the row to the south (row j0 itself for j0 = 0: not used there)

    const T* GU = static_cast<const T*>(p.GU) + a.off2;
    const T* GV = static_cast<const T*>(p.GV) + a.off2;
    const T* dxf = static_cast<const T*>(p.dx_fc) + a.off2;
    const T* dyc = static_cast<const T*>(p.dy_cf) + a.off2;
    const T* depth = static_cast<const T*>(p.depth);
    T* eta_out = static_cast<T*>(p.eta_out) + a.off2;
    T* U_out = static_cast<T*>(p.U_out) + a.off2;
    T* V_out = static_cast<T*>(p.V_out) + a.off2;
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const int j = j0 + min(r, nr - 1);
        const long long row = (long long)a.sx * j;
        T etap[W];
        sweep(row, yf[r + 1], yf[r + 2], yfw[r + 1], yfw[r + 2], etap, etaw, true);
        const cvec_t gu = chunk(GU, row), gv = chunk(GV, row), xfc = chunk(dxf, row), ycf = chunk(dyc, row);
        T gHu[W], gHv[W];
#pragma unroll
        for (int e = 0; e < W; ++e) gHu[e] = gHv[e] = g * depth[0];
        if constexpr (COUNTS) {
            typedef Counts<W> counts_t;
            if (p.nfc) {
                const counts_t n = *reinterpret_cast<const counts_t*>(p.nfc + (long long)a.Nx * j + e0);
#pragma unroll
                for (int e = 0; e < W; ++e) gHu[e] = g * depth[min(max(n[e], 0), a.Nz)];
            }
            if (p.ncf) {
                const counts_t n = *reinterpret_cast<const counts_t*>(p.ncf + (long long)a.Nx * j + e0);
#pragma unroll
                for (int e = 0; e < W; ++e) gHv[e] = g * depth[min(max(n[e], 0), a.Nz)];
            }
        }
        cvec_t eo, uo, vo;
        T west = etaw;                                             // eta'[i - 1, j]
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const T px = (etap[e] - west) / xfc[e];
            west = etap[e];
            const T py = (etap[e] - etas[e]) / ycf[e];
            eo[e] = etap[e];
            uo[e] = Ur[e] + dtau * (gu[e] - gHu[e] * px);
            const T vn = Vr[r][e] + dtau * (gv[e] - gHv[e] * py);
            vo[e] = j == 0 ? Vr[r][e] : vn;                         // the south wall row is carried
            etas[e] = etap[e];
        }
        if (r < nr) {
            *reinterpret_cast<cvec_t*>(eta_out + row + e0) = eo;
            *reinterpret_cast<cvec_t*>(U_out + row + e0) = uo;
            *reinterpret_cast<cvec_t*>(V_out + row + e0) = vo;
            if constexpr (AVG) {
                T* const bars[3] = { static_cast<T*>(p.eta_bar), static_cast<T*>(p.U_bar), static_cast<T*>(p.V_bar) };
                const cvec_t news[3] = { eo, uo, vo };
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    cvec_t* b = reinterpret_cast<cvec_t*>(bars[q] + a.off2 + row + e0);
                    cvec_t acc = *b;
#pragma unroll
                    for (int e = 0; e < W; ++e) acc[e] = acc[e] + wt * news[q][e];
                    *b = acc;
                }
            }
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_free_surface_last_error(void) { return tpg_last_error(); }

int tpg_free_surface_substep(void* eta_out, void* U_out, void* V_out, const void* eta_in, const void* U_in, const void* V_in, const void* GU,
                             const void* GV, void* eta_bar, void* U_bar, void* V_bar, const void* dy_fc, const void* dx_cf, const void* az_cc,
                             const void* dx_fc, const void* dy_cf, const void* depth_of_count, const int32_t* n_fc, const int32_t* n_cf,
                             double dtau, double g, double weight, int Nx, int Ny, int Nz, int Hx, int Hy2, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, 0, 0, 0, ft)) return rc;                              // ft, the sizes, Nx even; the halos are checked next
    if (Hx < 1 || Hy2 < 1) {
        tpg::set_error("the rule reads U[i+1, j] and V[i, j+1]: Hx >= 1 and Hy2 >= 1 needed (halo (%d,%d))", Hx, Hy2);
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (!eta_out || !U_out || !V_out || !eta_in || !U_in || !V_in || !GU || !GV) {
        tpg::set_error("null eta_out, U_out, V_out, eta_in, U_in, V_in, GU or GV");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (!dy_fc || !dx_cf || !az_cc || !dx_fc || !dy_cf) { tpg::set_error("null dy_fc, dx_cf, az_cc, dx_fc or dy_cf"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!depth_of_count) { tpg::set_error("null depth_of_count"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!eta_bar != !U_bar || !eta_bar != !V_bar) { tpg::set_error("eta_bar, U_bar and V_bar must be given together"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    const int NP = 16;
    const void* const planes[NP] = { eta_out, U_out, V_out, eta_bar, U_bar, V_bar, eta_in, U_in, V_in, GU, GV, dy_fc, dx_cf, az_cc, dx_fc, dy_cf };
    const char* const names[NP] = { "eta_out", "U_out", "V_out", "eta_bar", "U_bar", "V_bar", "eta_in", "U_in", "V_in", "GU", "GV",
                                    "dy_fc", "dx_cf", "az_cc", "dx_fc", "dy_cf" };
    const int NW = 6;                                              // the first NW are written
    for (int q = 0; q < NP; ++q)
        if (misaligned(esz, planes[q])) { tpg::set_error("%s pointer not aligned to its element type", names[q]); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(esz, depth_of_count)) { tpg::set_error("depth_of_count pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(4, n_fc, n_cf)) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    if ((long long)(Nx + 2ll * Hx) * (Ny + 2ll * Hy2) >= (1ll << 31)) { tpg::set_error("free surface: plane too large for 32-bit row offsets"); return TPG_ERR_UNSUPPORTED; }
    const Geom gm = tpg::make_geom(Nx, Ny, 1, Hx, Hy2, 0);
    const unsigned long long pbytes = (unsigned long long)gm.plane * esz;
    const unsigned long long cbytes = (unsigned long long)Nx * Ny * 4, dbytes = (unsigned long long)(Nz + 1) * esz;
    for (int o = 0; o < NW; ++o) {
        if (!planes[o]) continue;
        for (int q = 0; q < NP; ++q)
            if (q != o && planes[q] && arrays_overlap(planes[o], pbytes, planes[q], pbytes)) {
                tpg::set_error("%s overlaps %s (an item reads its neighbours' cells while their items write: eta, U, V ping-pong)", names[o], names[q]);
                return TPG_ERR_INVALID_ARGUMENT;
            }
        if (arrays_overlap(planes[o], pbytes, depth_of_count, dbytes) || (n_fc && arrays_overlap(planes[o], pbytes, n_fc, cbytes))
            || (n_cf && arrays_overlap(planes[o], pbytes, n_cf, cbytes))) {
            tpg::set_error("%s overlaps depth_of_count or a count plane", names[o]);
            return TPG_ERR_INVALID_ARGUMENT;
        }
    }
    if (Ny < 2) { tpg::set_error("free surface: Ny >= 2 needed (row 1 of V is the wall's)"); return TPG_ERR_UNSUPPORTED; }
    const long long tiles = (Ny + JT - 1) / JT;
    if (tiles * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("free surface: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    const FsPtrs p{ eta_out, U_out, V_out, eta_in, U_in, V_in, GU, GV, eta_bar, U_bar, V_bar, dy_fc, dx_cf, az_cc, dx_fc, dy_cf, depth_of_count, n_fc, n_cf };
    void* arrays[NP];
    int na = 0;
    for (int q = 0; q < NP; ++q) if (planes[q]) arrays[na++] = const_cast<void*>(planes[q]);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(gm, arrays, na);
        const int cpr = Nx / cp.W;
        const FsArgs a{ Nx, Ny, Nz, gm.sx, cpr, (int)(tiles * cpr), interior2(gm), (double)(T)dtau, (double)(T)g, (double)(T)weight };
        dim3 grid((unsigned)((a.items + 255) / 256));
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto averaging = [&](auto counts) {
                constexpr bool COUNTS = decltype(counts)::value;
                if (eta_bar) hipLaunchKernelGGL((k_free_surface_substep<T, W, GEN, COUNTS, true>), grid, dim3(256), 0, st, p, a);
                else         hipLaunchKernelGGL((k_free_surface_substep<T, W, GEN, COUNTS, false>), grid, dim3(256), 0, st, p, a);
            };
            if (n_fc || n_cf) averaging(std::true_type{});
            else              averaging(std::false_type{});
        });
        return tpg::launch_status("k_free_surface_substep");
    });
}

}  // extern "C"
