// tpg_immersed.hip -- grid-fitted immersed boundary: the column count planes (tpg_immersed_column_counts) and the store-only mask pass
// (tpg_mask_immersed_fields) for gfx950.
//
// Oceananigans' ImmersedBoundaryGrid(grid, GridFittedBottom(bottom_height)) and mask_immersed_field!(field, value) [recalled; parity
// unpinned: Oceananigans' source is not at hand, the rule is written down here and in tests/immersed_ref.py].  Grid Nz levels, z centres
// zc[1..Nz] strictly increasing, h[i, j] the bottom height at (Center, Center) AFTER its halo fill (zipper + periodic x, on a band the seam):
//     immersed_cell(i, j, k) = zc[k] <= h[i, j]                 compared in the grid's type; c[i, j] = #{k : zc[k] <= h[i, j]}, 0..Nz
//     inactive_cell          = immersed_cell, or k < 1, or k > Nz, or j < 1 where the south side is a wall (c = Nz there)
//     peripheral node        = ANY cell it touches is inactive: {i, i-1 if x-Face} x {j, j-1 if y-Face} x {k, k-1 if z-Face}
// x is periodic: cell i = 0 is h's filled west halo column; row j = 0 of a band that is not the southernmost is h's seam halo row; no
// node of the interior touches a cell with j > Ny (the zipper enters through h's own fill, which makes row Ny of h mirror-symmetric).
// Per horizontal location the masked levels of a column are therefore a PREFIX, and one int32 plane over the interior describes them:
//     n_cc = c    n_fc[i, j] = max(c[i, j], c[i-1, j])    n_cf[i, j] = max(c[i, j], c[i, j-1])    n_ff = max of the four
// a z-Center field is masked for k <= n, a z-Face field for k <= min(n + 1, Nz) (grid Nz: its level Nz + 1 is not visited).
//
// The mask writes `value` to the peripheral nodes i = 1..Nx, j = 1..Ny of the fields and touches nothing else: no halo cell, no unmasked
// cell.  It issues NO LOAD FROM A FIELD (Oceananigans computes ifelse(mask, value, c) on every cell; storing the masked cells alone yields
// the same array).  A PRE-PASS of the halo fill, ahead of the Open faces: mask -> Open faces -> horizontal fill -> ... (an Open bottom value
// of w overwrites the mask's value at k = 1, as in Oceananigans' update_state! [recalled]).
//
// HBM-bound stores, no arithmetic.  A work item owns one 16-B chunk of interior columns of one row j: it reads the chunk's counts once
// (count planes are dense, so they sit at the chunk's own column offset; 4-B aligned) and walks the levels upwards with stores one plane
// apart -- whole 16-B vector stores while every element of the chunk is masked, single element stores for the levels where only some are,
// nothing above.  grid.y = field (wave-uniform table reads).  Chunks cover the interior columns only (the x halos are the fill's): the
// plain form needs Hx and Nx whole chunks and 16-B aligned fields (chunk_plan), everything else (halo 5, offset pointers, Float32 rows
// with Nx = 2 mod 4) takes the element-aligned GEN form of the same chunks.
//
// Two things are compile-time switches until they are timed (bench_immersed.py --product-lib): -DTPG_IMMERSED_FORM_B=1 builds the
// other decomposition, a work item per (chunk, level) pair (k_mask_immersed_levels), behind the same entry point; -DTPG_IMMERSED_NT=1 gives
// the stores of the default form the non-temporal hint (the horizontal fill reads rows this pass wrote: the question tpg_open.hip records).
#include "tpg_launch.hpp"

#ifndef TPG_IMMERSED_FORM_B
#define TPG_IMMERSED_FORM_B 0
#endif
#ifndef TPG_IMMERSED_NT
#define TPG_IMMERSED_NT 0
#endif

namespace {

#if TPG_IMMERSED_NT
#define TPG_MASK_STORE(p, v) __builtin_nontemporal_store(v, p)
#else
#define TPG_MASK_STORE(p, v) (*(p) = (v))
#endif

struct MaskTable {
    void* ptr[TPG_MAX_FIELDS];
    const int32_t* counts[TPG_MAX_FIELDS];
    double value[TPG_MAX_FIELDS];          // T values held in a double
    int zloc[TPG_MAX_FIELDS];
};

struct MaskArgs {
    int Nx, Ny, Nz, Hx, Hy, Hz, sx;
    int cpr;                               // chunks per interior row
    long long plane;                       // sx * sy
};

template <int W> struct Counts { typedef int type __attribute__((ext_vector_type(W), aligned(4))); };

template <typename T, int W, bool GEN>
__global__ __launch_bounds__(256) void k_mask_immersed(MaskTable t, MaskArgs a)
{
    typedef typename Vec<T, W>::aligned_t vec_t;
    typedef typename Vec<T, W>::loose_t lvec_t;
    typedef typename std::conditional<GEN, lvec_t, vec_t>::type cvec_t;
    const int f = blockIdx.y;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.Ny * a.cpr) return;
    const int j = item / a.cpr;
    const int e0 = (item - j * a.cpr) * W;                         // first interior column of the chunk (0-based)
    const int zl = t.zloc[f];
    const int top = a.Nz - zl;                                     // a z-Face field's last level is not visited
    const typename Counts<W>::type n = *reinterpret_cast<const typename Counts<W>::type*>(t.counts[f] + (long long)a.Nx * j + e0);
    int m[W], lo = top, hi = 0;                                    // masked levels per element, clamped to the levels the field has
#pragma unroll
    for (int e = 0; e < W; ++e) {
        m[e] = min(n[e] + zl, top);
        lo = min(lo, m[e]);
        hi = max(hi, m[e]);
    }
    const T v = (T)t.value[f];
    T* p = static_cast<T*>(t.ptr[f]) + a.plane * a.Hz + (long long)a.sx * (a.Hy + j) + a.Hx + e0;
    int k = 0;
    for (; k < lo; ++k, p += a.plane) TPG_MASK_STORE(reinterpret_cast<cvec_t*>(p), (cvec_t)(v));
    for (; k < hi; ++k, p += a.plane) {
#pragma unroll
        for (int e = 0; e < W; ++e)
            if (k < m[e]) TPG_MASK_STORE(p + e, v);
    }
}

#if TPG_IMMERSED_FORM_B
// form (b): a work item is one (chunk, level) pair
template <typename T, int W, bool GEN>
__global__ __launch_bounds__(256) void k_mask_immersed_levels(MaskTable t, MaskArgs a)
{
    typedef typename Vec<T, W>::aligned_t vec_t;
    typedef typename Vec<T, W>::loose_t lvec_t;
    typedef typename std::conditional<GEN, lvec_t, vec_t>::type cvec_t;
    const int f = blockIdx.y;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = a.Ny * a.cpr;
    const int zl = t.zloc[f];
    const int top = a.Nz - zl;
    const int k = item / per;
    if (k >= top) return;
    const int r = item - k * per;
    const int j = r / a.cpr;
    const int e0 = (r - j * a.cpr) * W;
    const typename Counts<W>::type n = *reinterpret_cast<const typename Counts<W>::type*>(t.counts[f] + (long long)a.Nx * j + e0);
    int m[W], lo = top, hi = 0;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        m[e] = min(n[e] + zl, top);
        lo = min(lo, m[e]);
        hi = max(hi, m[e]);
    }
    if (k >= hi) return;
    const T v = (T)t.value[f];
    T* p = static_cast<T*>(t.ptr[f]) + a.plane * (a.Hz + k) + (long long)a.sx * (a.Hy + j) + a.Hx + e0;
    if (k < lo) { *reinterpret_cast<cvec_t*>(p) = (cvec_t)(v); return; }
#pragma unroll
    for (int e = 0; e < W; ++e)
        if (k < m[e]) p[e] = v;
}
#endif

// one thread per interior (i, j): the counts of the up to four cells the four horizontal locations touch
template <typename T>
__global__ __launch_bounds__(256) void k_column_counts(const T* __restrict__ h, const T* __restrict__ zc, int wall,
                                                       int32_t* n_cc, int32_t* n_fc, int32_t* n_cf, int32_t* n_ff,
                                                       int Nx, int Ny, int Nz, int Hx, int Hy)
{
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= Nx * Ny) return;
    const int j = item / Nx, i = item - j * Nx;                    // 0-based interior indices
    const int sx = Nx + 2 * Hx;
    const bool west = n_fc || n_ff, south = n_cf || n_ff;
    const bool row0 = south && !(wall && j == 0);                  // row j - 1 is read: an interior row, or the seam halo row of a band
    const T* hp = h + (long long)sx * (Hy + j) + Hx + i;
    const T h00 = hp[0];
    const T h10 = west ? hp[-1] : h00;
    const T h01 = row0 ? hp[-sx] : h00;
    const T h11 = (west && row0) ? hp[-sx - 1] : h01;
    int c00 = 0, c10 = 0, c01 = 0, c11 = 0;
    for (int k = 0; k < Nz; ++k) {
        const T z = zc[k];
        c00 += z <= h00; c10 += z <= h10; c01 += z <= h01; c11 += z <= h11;
    }
    if (south && !row0) c01 = c11 = Nz;                            // j - 1 < 1 behind a wall: inactive at every level
    if (n_cc) n_cc[item] = c00;
    if (n_fc) n_fc[item] = max(c00, c10);
    if (n_cf) n_cf[item] = max(c00, c01);
    if (n_ff) n_ff[item] = max(max(c00, c10), max(c01, c11));
}

}  // namespace

extern "C" {

int tpg_immersed_column_counts(const void* bottom_height, const void* z_centers, int south_is_wall,
                               int32_t* n_cc, int32_t* n_fc, int32_t* n_cf, int32_t* n_ff,
                               int Nx, int Ny, int Nz, int Hx, int Hy, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, 0, ft)) return rc;
    if (!bottom_height || !z_centers) { tpg::set_error("null bottom_height or z_centers"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    if ((uintptr_t)bottom_height % esz || (uintptr_t)z_centers % esz) {
        tpg::set_error("bottom_height or z_centers pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (((uintptr_t)n_cc | (uintptr_t)n_fc | (uintptr_t)n_cf | (uintptr_t)n_ff) % 4) {
        tpg::set_error("count plane pointer not aligned to int32");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if ((n_fc || n_ff) && Hx < 1) { tpg::set_error("n_fc / n_ff read cell i = 0 from the west halo column: Hx >= 1 needed (Hx = %d)", Hx); return TPG_ERR_UNSUPPORTED; }
    if ((n_cf || n_ff) && !south_is_wall && Hy < 1) {
        tpg::set_error("n_cf / n_ff without a south wall read row j = 0 from the seam halo row: Hy >= 1 needed (Hy = %d)", Hy);
        return TPG_ERR_UNSUPPORTED;
    }
    if ((long long)Nx * Ny >= (1ll << 31) - 256) { tpg::set_error("count planes too large for 32-bit work-item indexing"); return TPG_ERR_UNSUPPORTED; }
    if (!n_cc && !n_fc && !n_cf && !n_ff) return TPG_OK;
    dim3 grid((unsigned)(((long long)Nx * Ny + 255) / 256));
    dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        hipLaunchKernelGGL((k_column_counts<T>), grid, dim3(256), 0, tpg::as_stream(stream), static_cast<const T*>(bottom_height),
                           static_cast<const T*>(z_centers), south_is_wall ? 1 : 0, n_cc, n_fc, n_cf, n_ff, Nx, Ny, Nz, Hx, Hy);
    });
    return tpg::launch_status("k_column_counts");
}

int tpg_mask_immersed_fields(void* const fields[], int nfields, const int32_t* const counts[], const int8_t zloc[], const double values[],
                             int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc) return rc;
    if (!counts || !zloc || !values) { tpg::set_error("null counts, zloc or values table"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    for (int f = 0; f < nfields; ++f) {
        if (!counts[f]) { tpg::set_error("field %d: null count plane", f); return TPG_ERR_INVALID_ARGUMENT; }
        if (zloc[f] != TPG_CENTER && zloc[f] != TPG_FACE) { tpg::set_error("field %d: zloc = %d is neither TPG_CENTER nor TPG_FACE", f, (int)zloc[f]); return TPG_ERR_INVALID_ARGUMENT; }
        if ((uintptr_t)fields[f] % esz) { tpg::set_error("field %d: pointer not aligned to its element type", f); return TPG_ERR_INVALID_ARGUMENT; }
        if ((uintptr_t)counts[f] % 4) { tpg::set_error("field %d: count plane pointer not aligned to int32", f); return TPG_ERR_INVALID_ARGUMENT; }
    }
    if ((long long)Nx * Ny * (TPG_IMMERSED_FORM_B ? Nz : 1) >= (1ll << 31) - 256) { tpg::set_error("mask too large for 32-bit work-item indexing"); return TPG_ERR_UNSUPPORTED; }
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    hipStream_t st = tpg::as_stream(stream);
    return for_each_batch(nfields, [&](int f0, int n) {
        MaskTable t;
        for (int f = 0; f < n; ++f) {
            t.ptr[f] = fields[f0 + f];
            t.counts[f] = counts[f0 + f];
            t.value[f] = values[f0 + f];
            t.zloc[f] = zloc[f0 + f];
        }
        return dispatch_ft(ft, [&](auto ty) {
            typedef decltype(ty) T;
            const ChunkPlan cp = chunk_plan<T>(g, fields + f0, n);
            const MaskArgs a{ Nx, Ny, Nz, Hx, Hy, Hz, g.sx, Nx / cp.W, g.plane };
#if TPG_IMMERSED_FORM_B
            dim3 grid((unsigned)(((long long)Nz * Ny * a.cpr + 255) / 256), (unsigned)n);
            dispatch_chunk<T>(cp.W, cp.gen, [&](auto w, auto gen) {
                hipLaunchKernelGGL((k_mask_immersed_levels<T, decltype(w)::value, decltype(gen)::value>), grid, dim3(256), 0, st, t, a);
            });
#else
            dim3 grid((unsigned)(((long long)Ny * a.cpr + 255) / 256), (unsigned)n);
            dispatch_chunk<T>(cp.W, cp.gen, [&](auto w, auto gen) {
                hipLaunchKernelGGL((k_mask_immersed<T, decltype(w)::value, decltype(gen)::value>), grid, dim3(256), 0, st, t, a);
            });
#endif
            return tpg::launch_status("k_mask_immersed");
        });
    });
}

}  // extern "C"
