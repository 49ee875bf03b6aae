// tpg_barotropic.hip -- the two ends of a split-explicit free surface's sub-cycle on the 3-D velocities, for gfx950: the barotropic mode
// (tpg_barotropic_mode) before it and the velocity correction (tpg_barotropic_correction) after it.
// [recalled: Oceananigans' `compute_barotropic_mode!` and `barotropic_split_explicit_corrector!`; parity unpinned, like every operator here.]
//
// Fields
// - `u` at (Face, Center, Center) and `v` at (Center, Face, Center): padded parents of geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
// - `U`, `V`, `Ubar`, `Vbar`: 2-D padded planes of `(Ny + 2 Hy2) x (Nx + 2 Hx)`: the same `Hx`, so the same row pitch `sx` as the 3-D fields,
//   and THEIR OWN north / south halo `Hy2` (the free surface's fields live on the extended-halo grid).  First interior cell: `sx Hy2 + Hx`.
// - `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]` in the field type.  `depth_of_count`: `Nz + 1` values in the field type, `depth_of_count[n]` the depth of a
//   column whose lowest `n` cells are immersed.
// The mode, for every interior column `i = 1..Nx`, `j = 1..Ny`, in the field type, in exactly this order, no contraction, every operation one
// correctly rounded IEEE operation:
//     Ubar[i,j] = dz_c[1] * u[i,j,1]
//     for k = 2..Nz:  Ubar[i,j] = Ubar[i,j] + dz_c[k] * u[i,j,k]
// and Vbar from v likewise.
// The correction, in place, for every interior node:
//     H = depth_of_count[min(n_fc[i,j], Nz)]        (n_fc NULL: depth_of_count[0])
//     c = (U[i,j] - Ubar[i,j]) / H                  one subtraction, one division, formed once per column
//     u[i,j,k] = u[i,j,k] + c      k = 1..Nz
// and v likewise with V, Vbar, n_cf.  `H = 0` divides by it, as the rule says.
// - Only interior cells are written (of Ubar / Vbar by the mode, of u / v by the correction); no halo cell of any array is read.  There is no
//   stencil: every halo width >= 0 is accepted.
// - Levels under an immersed bottom ARE read by the mode (a model's u, v are masked there), as tpg_w_from_continuity reads them.
//
// Both are HBM-bound streams, one field per grid.y, ONE launch for both fields.
// The mode: a work item is ONE chunk of W interior columns and walks ALL levels with the running sum in registers -- level segments would
// re-associate the sum, which is not the rule.  Only the add depends on the previous level; no load does: the loads of the next LOOKAHEAD
// levels are issued before the current level's add (the ring of tpg_continuity.hip, deeper: an item here holds one vector per level).
// The correction: `c` is a pure function of 2-D values, so an item is one chunk x a SEGMENT of consecutive levels, each segment re-forming
// `c`; the segment's levels go BATCH at a time, loads first, then adds and stores.  Items are numbered (segment, row, chunk), chunk fastest.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over all
// the arrays passed (the 2-D planes share sx and Hx, so their interior sits on the 16-B grid exactly when their pointer does).  Element
// offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
//
// Fused mask (a count plane given): u nodes k <= n_fc (v: n_cf) get `mask_value` (converted once to T) instead -- bit for bit what
// tpg_mask_immersed_fields leaves on u (plane fc, TPG_CENTER) and v (plane cf) after the unmasked call.
#include "tpg_operator.hpp"
#include "../../include/tripolar_hip_barotropic.h"

// compile-time switches of the A/B in profiles/barotropic/ (make BAROTROPIC_TAG=_la8 BAROTROPIC_FLAGS='-DTPG_BARO_LOOKAHEAD=8', -DTPG_BARO_SEG=16,
// -DTPG_BARO_BATCH=2 or -DTPG_BARO_NT=1).  Measured at 3600 x 1800 x 75: 2, 4 and 8 levels of look-ahead are one time (the mode runs at the
// time of tpg_field_extrema over the same cells), 12 and 16 take 2.4 times as long; an item of the correction that walks all 75 levels is
// 3 - 5 % faster than segments of 16 and 5 - 8 % faster than segments of 5 in Float64; 2, 4 and 8 levels per batch and non-temporal stores
// change nothing.
#ifndef TPG_BARO_LOOKAHEAD
#define TPG_BARO_LOOKAHEAD 4
#endif
#ifndef TPG_BARO_SEG
#define TPG_BARO_SEG 75
#endif
#ifndef TPG_BARO_BATCH
#define TPG_BARO_BATCH 4
#endif
#ifndef TPG_BARO_NT
#define TPG_BARO_NT 0
#endif

namespace {

constexpr int LA = TPG_BARO_LOOKAHEAD;     // the mode: levels whose loads are in flight ahead of the add
constexpr int SEG = TPG_BARO_SEG;          // the correction: levels per work item
constexpr int BATCH = TPG_BARO_BATCH;      // the correction: levels loaded before the first of them is stored
constexpr bool NT = TPG_BARO_NT;          // the correction: u and v go out in ordinary stores

struct ModePtrs {
    const void* src[2];                    // u and / or v, packed to the front
    void* dst[2];                          // Ubar / Vbar
    const void* dz;
};

struct CorrPtrs {
    void* f[2];                            // u and / or v, packed to the front
    const void* t[2];                      // U / V
    const void* tbar[2];                   // Ubar / Vbar
    const int32_t* n[2];                   // n_fc / n_cf, or null
    const void* depth;
};

struct BaroArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int rowitems;                          // Ny * cpr
    int items;                             // rowitems (the mode), segments x rowitems (the correction)
    long long plane;                       // sx * sy
    long long off3;                        // plane * Hz + sx * Hy + Hx: the first interior cell of a 3-D parent
    long long off2;                        // sx * Hy2 + Hx: the first interior cell of a 2-D plane
    double value;                          // the mask value (a T value held in a double)
};

template <typename T, int W, bool GEN>
__global__ __launch_bounds__(256) void k_barotropic_mode(ModePtrs p, BaroArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int j = item / a.cpr;                                    // interior row (0-based)
    const int e0 = (item - j * a.cpr) * W;                         // first interior column of the chunk (0-based)
    const long long row = (long long)a.sx * j + e0;
    const T* src = static_cast<const T*>(p.src[blockIdx.y]) + a.off3 + row;
    T* dst = static_cast<T*>(p.dst[blockIdx.y]) + a.off2 + row;
    const T* dz = static_cast<const T*>(p.dz);

    cvec_t ring[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) ring[s] = *reinterpret_cast<const cvec_t*>(src + a.plane * min(s, a.Nz - 1));
    cvec_t acc;
    for (int k0 = 0; k0 < a.Nz; k0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int k = k0 + s;
            if (k >= a.Nz) break;
            const cvec_t x = ring[s];
            if (k + LA < a.Nz) ring[s] = *reinterpret_cast<const cvec_t*>(src + a.plane * (k + LA));   // level k + LA goes out before level k's add
            const T d = dz[k];
            if (k == 0) {
#pragma unroll
                for (int e = 0; e < W; ++e) acc[e] = d * x[e];     // the first term is the product itself: +0 + (-0) would lose its sign
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) acc[e] = acc[e] + d * x[e];
            }
        }
    }
    *reinterpret_cast<cvec_t*>(dst) = acc;
}

template <typename T, int W, bool GEN, bool MASK>
__global__ __launch_bounds__(256) void k_barotropic_correction(CorrPtrs p, BaroArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int seg = item / a.rowitems;
    const int rem = item - seg * a.rowitems;
    const int j = rem / a.cpr;                                     // interior row (0-based)
    const int e0 = (rem - j * a.cpr) * W;                          // first interior column of the chunk (0-based)
    const int k0 = seg * SEG, k1 = min(k0 + SEG, a.Nz);            // the segment's levels (0-based)
    const long long row = (long long)a.sx * j + e0;

    // c of the chunk's columns, once per item
    const cvec_t t = *reinterpret_cast<const cvec_t*>(static_cast<const T*>(p.t[blockIdx.y]) + a.off2 + row);
    const cvec_t tb = *reinterpret_cast<const cvec_t*>(static_cast<const T*>(p.tbar[blockIdx.y]) + a.off2 + row);
    const T* depth = static_cast<const T*>(p.depth);
    const int32_t* counts = MASK ? p.n[blockIdx.y] : nullptr;      // one field of the two may have no plane
    int m[W];
    T c[W];
#pragma unroll
    for (int e = 0; e < W; ++e) m[e] = 0;
    if (MASK && counts) {
        const Counts<W> n = *reinterpret_cast<const Counts<W>*>(counts + (long long)a.Nx * j + e0);
#pragma unroll
        for (int e = 0; e < W; ++e) m[e] = min(max(n[e], 0), a.Nz);  // masked levels (0-based k < m); the index into depth_of_count
    }
#pragma unroll
    for (int e = 0; e < W; ++e) c[e] = (t[e] - tb[e]) / depth[m[e]];
    const T mv = (T)a.value;

    T* f = static_cast<T*>(p.f[blockIdx.y]) + a.off3 + row;
    for (int kb = k0; kb < k1; kb += BATCH) {
        cvec_t x[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) x[b] = *reinterpret_cast<const cvec_t*>(f + a.plane * min(kb + b, k1 - 1));
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            const int k = kb + b;
            if (k >= k1) break;
            cvec_t out;
#pragma unroll
            for (int e = 0; e < W; ++e) out[e] = (MASK && k < m[e]) ? mv : x[b][e] + c[e];
            store_chunk<NT>(reinterpret_cast<cvec_t*>(f + a.plane * k), out);
        }
    }
}

// the checks both calls start with, in this order
int check_shape(int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int Hy2, int ft)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (Hy2 < 0) { tpg::set_error("invalid north/south halo Hy2=%d of the 2-D planes", Hy2); return TPG_ERR_INVALID_ARGUMENT; }
    return TPG_OK;
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_barotropic_last_error(void) { return tpg_last_error(); }

int tpg_barotropic_mode(const void* u, const void* v, void* Ubar, void* Vbar, const void* dz_c, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                        int Hy2, int ft, void* stream)
{
    if (int rc = check_shape(Nx, Ny, Nz, Hx, Hy, Hz, Hy2, ft)) return rc;
    if (!u && !v && !Ubar && !Vbar) { tpg::set_error("u, v, Ubar and Vbar all null: nothing to compute"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!u != !Ubar) { tpg::set_error("u and Ubar must be given together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!v != !Vbar) { tpg::set_error("v and Vbar must be given together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!dz_c) { tpg::set_error("null dz_c"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    if (misaligned(esz, u, v, Ubar, Vbar)) {
        tpg::set_error("u, v, Ubar or Vbar pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (misaligned(esz, dz_c)) { tpg::set_error("dz_c pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz;                    // u, v
    const unsigned long long pbytes = (unsigned long long)g.sx * (Ny + 2ll * Hy2) * esz;                   // Ubar, Vbar
    void* const outs[2] = { Ubar, Vbar };
    const char* const names[2] = { "Ubar", "Vbar" };
    for (int o = 0; o < 2; ++o)
        if (outs[o] && ((u && arrays_overlap(outs[o], pbytes, u, bytes)) || (v && arrays_overlap(outs[o], pbytes, v, bytes)))) {
            tpg::set_error("%s overlaps u's or v's parent (every column reads cells while other columns write)", names[o]);
            return TPG_ERR_INVALID_ARGUMENT;
        }
    if (Ubar && Vbar && arrays_overlap(Ubar, pbytes, Vbar, pbytes)) { tpg::set_error("Ubar overlaps Vbar"); return TPG_ERR_INVALID_ARGUMENT; }
    if ((long long)Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("barotropic mode: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    ModePtrs p{};
    void* arrays[4];
    int nf = 0, na = 0;
    if (u) { p.src[nf] = u; p.dst[nf++] = Ubar; arrays[na++] = const_cast<void*>(u); arrays[na++] = Ubar; }
    if (v) { p.src[nf] = v; p.dst[nf++] = Vbar; arrays[na++] = const_cast<void*>(v); arrays[na++] = Vbar; }
    p.dz = dz_c;
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        const BaroArgs a{ Nx, Ny, Nz, g.sx, cpr, Ny * cpr, Ny * cpr, g.plane, interior3(g), (long long)g.sx * Hy2 + Hx, 0.0 };
        dim3 grid((unsigned)((a.items + 255) / 256), (unsigned)nf);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            hipLaunchKernelGGL((k_barotropic_mode<T, decltype(cw)::value, decltype(gen)::value>), grid, dim3(256), 0, st, p, a);
        });
        return tpg::launch_status("k_barotropic_mode");
    });
}

int tpg_barotropic_correction(void* u, void* v, const void* U, const void* V, const void* Ubar, const void* Vbar, const void* depth_of_count,
                              const int32_t* n_fc, const int32_t* n_cf, double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                              int Hy2, int ft, void* stream)
{
    if (int rc = check_shape(Nx, Ny, Nz, Hx, Hy, Hz, Hy2, ft)) return rc;
    if (!u && !v && !U && !V && !Ubar && !Vbar) { tpg::set_error("u, v, U, V, Ubar and Vbar all null: nothing to compute"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!u != !U || !u != !Ubar) { tpg::set_error("u, U and Ubar must be given together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!v != !V || !v != !Vbar) { tpg::set_error("v, V and Vbar must be given together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!depth_of_count) { tpg::set_error("null depth_of_count"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    if (misaligned(esz, u, v, U, V, Ubar, Vbar)) {
        tpg::set_error("u, v, U, V, Ubar or Vbar pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (misaligned(esz, depth_of_count)) { tpg::set_error("depth_of_count pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(4, n_fc, n_cf)) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz;                    // u, v
    const unsigned long long pbytes = (unsigned long long)g.sx * (Ny + 2ll * Hy2) * esz;                   // U, V, Ubar, Vbar
    const void* const planes[4] = { U, V, Ubar, Vbar };
    const char* const names[4] = { "U", "V", "Ubar", "Vbar" };
    for (int o = 0; o < 4; ++o)
        if (planes[o] && ((u && arrays_overlap(planes[o], pbytes, u, bytes)) || (v && arrays_overlap(planes[o], pbytes, v, bytes)))) {
            tpg::set_error("%s overlaps u's or v's parent (every column reads cells while other columns write)", names[o]);
            return TPG_ERR_INVALID_ARGUMENT;
        }
    if (u && v && arrays_overlap(u, bytes, v, bytes)) { tpg::set_error("u's parent overlaps v's: both are written"); return TPG_ERR_INVALID_ARGUMENT; }
    const long long segs = (Nz + SEG - 1) / SEG;
    if (segs * Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("barotropic correction: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    CorrPtrs p{};
    void* arrays[6];
    int nf = 0, na = 0;
    if (u) { p.f[nf] = u; p.t[nf] = U; p.tbar[nf] = Ubar; p.n[nf++] = n_fc; arrays[na++] = u; arrays[na++] = const_cast<void*>(U); arrays[na++] = const_cast<void*>(Ubar); }
    if (v) { p.f[nf] = v; p.t[nf] = V; p.tbar[nf] = Vbar; p.n[nf++] = n_cf; arrays[na++] = v; arrays[na++] = const_cast<void*>(V); arrays[na++] = const_cast<void*>(Vbar); }
    p.depth = depth_of_count;
    const bool mask = (u && n_fc) || (v && n_cf);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        const BaroArgs a{ Nx, Ny, Nz, g.sx, cpr, Ny * cpr, (int)(segs * Ny * cpr), g.plane, interior3(g),
                          (long long)g.sx * Hy2 + Hx, mask ? (double)(T)mask_value : 0.0 };
        dim3 grid((unsigned)((a.items + 255) / 256), (unsigned)nf);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            if (mask) hipLaunchKernelGGL((k_barotropic_correction<T, W, GEN, true>), grid, dim3(256), 0, st, p, a);
            else      hipLaunchKernelGGL((k_barotropic_correction<T, W, GEN, false>), grid, dim3(256), 0, st, p, a);
        });
        return tpg::launch_status("k_barotropic_correction");
    });
}

}  // extern "C"
