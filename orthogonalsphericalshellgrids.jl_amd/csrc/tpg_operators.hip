// tpg_operators.hip -- diagnostic operators on model fields for gfx950: the vertical vorticity at (Face, Face, Center)
// (tpg_vertical_vorticity).
//
// What the reference's model drivers create with VerticalVorticityField(model) and write on every output (examples/bickley_jet.jl:57,79;
// examples/distributed_bickley_jet.jl:59,83).  Oceananigans' operator [recalled; parity unpinned: its source is not at hand, the rule is
// written down here, in include/tripolar_hip_operators.h and in tests/vorticity_ref.py].  For every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz, in
// the field type, in exactly this order, no contraction (-ffp-contract=off), correctly rounded division:
//     a = dy_cf[i,j] * v[i,j,k]     b = dy_cf[i-1,j] * v[i-1,j,k]     c = dx_fc[i,j] * u[i,j,k]     d = dx_fc[i,j-1] * u[i,j-1,k]
//     zeta[i,j,k] = ((a - b) - (c - d)) / az_ff[i,j]
// Cells read: u[i, j-1..j, k], v[i-1..i, j, k] and the same cells of dx_fc / dy_cf, az_ff[i, j]: one halo column to the west, one halo row
// to the south (Hx >= 1, Hy >= 1; on a latitude band row 0 is the exchanged seam row).  Only interior cells of zeta are written.
//
// HBM-bound: two streams read, one written, 3 s bytes per cell, plus the three metric planes.  At 3600 x 1800 those planes are 52 MB each:
// walking the rows level by level puts 156 MB of metrics and 156 MB of field data between two uses of a metric line -- more than the
// 256 MiB Infinity Cache keeps -- so the planes would come from HBM again on every level (11.7 GB beside 13 GB of fields at 75 levels).
// Hence the work item: ONE chunk of W interior columns x JT rows x a SEGMENT of consecutive levels.  The item loads its metric values
// once -- dy_cf at the chunk and one column to the west, dx_fc of rows j0-1 .. j0+JT-1, az_ff (the division stays a division: a
// reciprocal is not bit-identical) -- keeps them in registers and walks the levels of its segment innermost, one plane apart: per level
// JT+1 rows of u ((JT+1)/JT reads of u), JT rows of v and the west neighbour of each (the same cache line), JT rows of zeta.  The product
// b of element e > 0 IS the product a of element e - 1, and the product d of row r IS the product c of row r - 1: each is formed once.
// Items are numbered (row tile, chunk) with the chunk fastest, 256 to a block; grid.y is the level segment.  Segments exist for the tail
// only: a block that walks all 75 levels runs for a third of the whole pass at the headline size (3164 blocks on ~1000 resident), so the
// last round would idle most of the device; the metric planes are re-read once per segment, 156 MB against 2.6 GB of fields per 15 levels.
// One level per segment IS the level-outer order (the test library's TPG_VORTICITY_LEVELS = 1; profiles/vorticity/ holds the comparison).
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise (odd Hx, Float32 rows with
// Nx = 2 mod 4 in 8-B chunks, offset pointers): chunk_plan's plain / GEN split.  No atomics, no LDS, no inter-block hand-off, nothing
// allocated, no host wait.
//
// Fused mask (n_ff given): nodes k <= n_ff[i,j] get `mask_value` (converted once to T) -- what tpg_mask_immersed_fields writes to a
// (Face, Face, Center) field -- and nothing is computed there: a chunk row whose elements are all masked at a level is a single vector store
// and loads nothing; a row with some masked elements is computed whole and the masked elements replaced, so nothing a masked node would have
// read (a NaN under land) reaches the output.
#include "tpg_operator.hpp"
#include "../../include/tripolar_hip_operators.h"

// compile-time switches of the A/B in profiles/vorticity/ (make OPERATORS_FLAGS='-DTPG_VORT_JT=8' or -DTPG_VORT_NT=0).  Measured at
// 3600 x 1800 x 75, halo 4, Float64 / Float32: streaming stores 2.66 / 1.25 ms against 2.74 / 1.30 ms with ordinary stores (zeta is not read
// again by this pass, and its lines then do not push the u rows two neighbouring tiles share out of the caches); 8 rows per item with
// streaming stores 2.52 / 1.25 ms, at 142 - 213 VGPRs (2 - 3 waves per SIMD): not taken, a follow-up.
#ifndef TPG_VORT_JT
#define TPG_VORT_JT 4
#endif
#ifndef TPG_VORT_NT
#define TPG_VORT_NT 1
#endif

namespace {

constexpr int JT = TPG_VORT_JT;            // rows per work item
constexpr bool NT = TPG_VORT_NT;          // zeta goes out in streaming stores
constexpr int VORT_LEVELS = 16;            // levels per segment (the product's; TPG_VORTICITY_LEVELS in the test library)

struct VortPtrs {
    const void *u, *v;
    void* zeta;
    const void *dx, *dy, *az;
    const int32_t* nff;
};

struct VortArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int items;                             // row tiles x cpr
    int levels;                            // levels per segment (grid.y = segment)
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double value;                          // the mask value (a T value held in a double)
};

template <typename T, int W, bool GEN, bool MASK>
__global__ __launch_bounds__(256) void k_vertical_vorticity(VortPtrs p, VortArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int e0 = (item - tile * a.cpr) * W;                      // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const int k0 = blockIdx.y * a.levels, k1 = min(k0 + a.levels, a.Nz);

    // the tile's metrics, once.  Rows past the interior's last are never used: their loads are clamped onto the last row
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    const T* dx = static_cast<const T*>(p.dx) + m0;
    const T* dy = static_cast<const T*>(p.dy) + m0;
    const T* az = static_cast<const T*>(p.az) + m0;
    T dyc[JT][W], dyw[JT], dxr[JT + 1][W], azr[JT][W];
    int lo[JT], m[JT][W];
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const int rr = min(r, nr - 1);
        const cvec_t y = *reinterpret_cast<const cvec_t*>(dy + a.sx * rr);
        const cvec_t z = *reinterpret_cast<const cvec_t*>(az + a.sx * rr);
        dyw[r] = dy[a.sx * rr - 1];                                // dy_cf[i - 1, j] of the chunk's first column
#pragma unroll
        for (int e = 0; e < W; ++e) { dyc[r][e] = y[e]; azr[r][e] = z[e]; }
        lo[r] = 0;
        if constexpr (MASK) {
            const Counts<W> n = *reinterpret_cast<const Counts<W>*>(p.nff + (long long)a.Nx * (j0 + rr) + e0);
            lo[r] = a.Nz;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                m[r][e] = min(n[e], a.Nz);                         // masked levels (0-based k < m) of the node's column
                lo[r] = min(lo[r], m[r][e]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r <= JT; ++r) {
        const cvec_t x = *reinterpret_cast<const cvec_t*>(dx + a.sx * (min(r, nr) - 1));      // rows j0 - 1 .. j0 + JT - 1
#pragma unroll
        for (int e = 0; e < W; ++e) dxr[r][e] = x[e];
    }

    const long long f0 = a.off3 + (long long)a.sx * j0 + e0;
    const T* u = static_cast<const T*>(p.u) + f0;
    const T* v = static_cast<const T*>(p.v) + f0;
    T* zeta = static_cast<T*>(p.zeta) + f0;
    const T mv = (T)a.value;
    for (int k = k0; k < k1; ++k) {
        const long long o3 = a.plane * k;
        T d[W];                                                    // dx_fc[i, j-1] * u[i, j-1, k]: the previous row's c
        bool have = false;
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            if (r >= nr) break;
            const long long o = o3 + a.sx * r;
            if (MASK && k < lo[r]) {                               // every node of the chunk row is masked: nothing is read
                store_chunk<NT>(reinterpret_cast<cvec_t*>(zeta + o), (cvec_t)(mv));
                have = false;
                continue;
            }
            if (!have) {
                const cvec_t us = *reinterpret_cast<const cvec_t*>(u + o - a.sx);
#pragma unroll
                for (int e = 0; e < W; ++e) d[e] = dxr[r][e] * us[e];
            }
            const cvec_t uu = *reinterpret_cast<const cvec_t*>(u + o);
            const cvec_t vv = *reinterpret_cast<const cvec_t*>(v + o);
            T b = dyw[r] * v[o - 1];                               // dy_cf[i-1, j] * v[i-1, j, k]; for e > 0 it is the a of e - 1
            cvec_t out;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const T aa = dyc[r][e] * vv[e];
                const T c = dxr[r + 1][e] * uu[e];
                const T z = ((aa - b) - (c - d[e])) / azr[r][e];
                out[e] = (MASK && k < m[r][e]) ? mv : z;
                b = aa;
                d[e] = c;
            }
            have = true;
            store_chunk<NT>(reinterpret_cast<cvec_t*>(zeta + o), out);
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_operators_last_error(void) { return tpg_last_error(); }

int tpg_vertical_vorticity(const void* u, const void* v, void* zeta, const void* dx_fc, const void* dy_cf, const void* az_ff,
                           const int32_t* n_ff, double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (!u || !v || !zeta) { tpg::set_error("null u, v or zeta"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!dx_fc || !dy_cf || !az_ff) { tpg::set_error("null dx_fc, dy_cf or az_ff"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    if (misaligned(esz, u, v, zeta)) { tpg::set_error("u, v or zeta pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(esz, dx_fc, dy_cf, az_ff)) {
        tpg::set_error("dx_fc, dy_cf or az_ff pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if ((uintptr_t)n_ff % 4) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz;
    if (arrays_overlap(zeta, bytes, u, bytes) || arrays_overlap(zeta, bytes, v, bytes)) {
        tpg::set_error("zeta's parent overlaps u's or v's (every node reads cells its neighbours' nodes write)");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (Hx < 1 || Hy < 1) {
        tpg::set_error("the rule reads u[i, j-1] and v[i-1, j]: Hx >= 1 and Hy >= 1 needed (halo (%d,%d))", Hx, Hy);
        return TPG_ERR_UNSUPPORTED;
    }
    const long long tiles = (Ny + JT - 1) / JT;
    if (tiles * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("vorticity: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    int levels = tpg::config().vorticity_levels > 0 ? tpg::config().vorticity_levels : VORT_LEVELS;
    if ((Nz + levels - 1) / levels > 65535) levels = (Nz + 65534) / 65535;           // grid.y
    const VortPtrs p{ u, v, zeta, dx_fc, dy_cf, az_ff, n_ff };
    hipStream_t st = tpg::as_stream(stream);
    void* const arrays[6] = { const_cast<void*>(u), const_cast<void*>(v), zeta, const_cast<void*>(dx_fc), const_cast<void*>(dy_cf), const_cast<void*>(az_ff) };
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, 6);
        const int cpr = Nx / cp.W;
        const VortArgs a{ Nx, Ny, Nz, g.sx, cpr, (int)(tiles * cpr), levels, g.plane, interior2(g), interior3(g), (double)(T)mask_value };
        dim3 grid((unsigned)((a.items + 255) / 256), (unsigned)((Nz + levels - 1) / levels));
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto w, auto gen) {
            if (n_ff) hipLaunchKernelGGL((k_vertical_vorticity<T, decltype(w)::value, decltype(gen)::value, true>), grid, dim3(256), 0, st, p, a);
            else      hipLaunchKernelGGL((k_vertical_vorticity<T, decltype(w)::value, decltype(gen)::value, false>), grid, dim3(256), 0, st, p, a);
        });
        return tpg::launch_status("k_vertical_vorticity");
    });
}

}  // extern "C"
