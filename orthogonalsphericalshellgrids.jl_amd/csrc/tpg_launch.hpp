// tpg_launch.hpp -- the host-side launch layer of the halo passes (tpg_zipper.hip, tpg_bounded.hip, tpg_value_gradient.hip, tpg_testabi.hip;
// tpg_geometry.hip for the dispatch helpers): every rule that chooses a kernel instantiation or shapes a call, once -- element type, (W, GEN)
// chunk form, Hy, field batches, the 16-B grid test, the argument checks, the timing-event scope -- and the launchers of the fill kernels.
#pragma once
#include "tpg_zipper_kernels.hpp"

namespace {

// ft (validated by tpg::check_geom) -> f(double()) / f(float()): the argument is a type tag, `decltype(ty)` the element type
template <typename F>
auto dispatch_ft(int ft, F&& f) { return ft == TPG_F64 ? f(double()) : f(float()); }

// THE (T, W, GEN) instantiations that exist, as f(integral_constant<int, W>, bool_constant<GEN>): 16-B chunks (W = 2 doubles / 4 floats)
// plain and GEN; Float32 8-B chunks (W = 2) GEN only
template <typename T, typename F>
auto dispatch_chunk(int W, bool gen, F&& f)
{
    constexpr int WMAX = 16 / (int)sizeof(T);
    if (!gen) return f(std::integral_constant<int, WMAX>{}, std::false_type{});
    if (W == 2) return f(std::integral_constant<int, 2>{}, std::true_type{});
    return f(std::integral_constant<int, WMAX>{}, std::true_type{});
}

// Hy -> f(std::integral_constant<int, HY>): 1..7 as themselves, everything else as 8 (the kernels exist for HY = 1..8; callers send those)
template <int HY = 1, typename F>
auto dispatch_hy(int Hy, F&& f)
{
    if constexpr (HY < 8) { if (Hy != HY) return dispatch_hy<HY + 1>(Hy, f); }
    return f(std::integral_constant<int, HY>{});
}

// f(f0, n) per batch of at most TPG_MAX_FIELDS fields (one kernarg table); stops at the first non-zero status and returns it
template <typename F>
int for_each_batch(int nfields, F&& f)
{
    for (int f0 = 0; f0 < nfields; f0 += TPG_MAX_FIELDS)
        if (int rc = f(f0, nfields - f0 < TPG_MAX_FIELDS ? nfields - f0 : TPG_MAX_FIELDS)) return rc;
    return TPG_OK;
}

// every row start, the n fields and every further pointer on the 16-B grid: the aligned (plain) access types are allowed
template <typename... P>
bool rows_on_16B_grid(size_t row_bytes, void* const fields[], int n, P... more)
{
    uintptr_t low = ((uintptr_t)row_bytes | ... | (uintptr_t)more);
    for (int f = 0; f < n; ++f) low |= (uintptr_t)fields[f];
    return low % 16 == 0;
}

// the checks every fill entry point starts with, in this order
int check_call(void* const fields[], int nfields, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (!fields || nfields < 1) { tpg::set_error("no fields"); return TPG_ERR_INVALID_ARGUMENT; }
    for (int f = 0; f < nfields; ++f) if (!fields[f]) { tpg::set_error("null field %d", f); return TPG_ERR_INVALID_ARGUMENT; }
    return TPG_OK;
}

// _fill_north_halo! has methods for the four (x, y) location pairs only (zipper_boundary_condition.jl:140-155)
int check_locations(const int8_t xloc[], const int8_t yloc[], const int32_t sign[], int nfields)
{
    if (!xloc || !yloc || !sign) { tpg::set_error("null location/sign table"); return TPG_ERR_INVALID_ARGUMENT; }
    for (int f = 0; f < nfields; ++f)
        if ((xloc[f] != TPG_CENTER && xloc[f] != TPG_FACE) || (yloc[f] != TPG_CENTER && yloc[f] != TPG_FACE)) {
            tpg::set_error("field %d: no zipper method for location (%d,%d)", f, xloc[f], yloc[f]);
            return TPG_ERR_INVALID_ARGUMENT;
        }
    return TPG_OK;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));      // 16 B of any element type (k_periodic_x_vec, k_pack)

// one batch (n <= TPG_MAX_FIELDS) of the caller's tables; item0 all zero (grid.y = field; zipper_batch sets its own prefix sums)
void fill_field_table(FieldTable& t, void* const fields[], const int8_t xloc[], const int8_t yloc[], const int32_t sign[], int n)
{
    t.nfields = n;
    for (int f = 0; f < n; ++f) { t.ptr[f] = fields[f]; t.xloc[f] = xloc[f]; t.yloc[f] = yloc[f]; t.sign[f] = sign[f]; t.item0[f] = 0; }
    t.item0[n] = 0;
}

// held by the *_timed entry points for the duration of the call: the FIRST TPG_LAUNCH of the call carries the events
struct TimedScope {
    TimedScope(void* start, void* stop) { tpg::ev_start = static_cast<hipEvent_t>(start); tpg::ev_stop = static_cast<hipEvent_t>(stop); }
    ~TimedScope() { tpg::ev_start = tpg::ev_stop = nullptr; }
};

#define TPG_LAUNCH(kernel, grid, block, stream, ...)                                                            \
    do {                                                                                                        \
        if (tpg::ev_start || tpg::ev_stop) {                                                                    \
            hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, tpg::ev_start, tpg::ev_stop, 0, __VA_ARGS__); \
            tpg::ev_start = tpg::ev_stop = nullptr;                                                             \
        } else                                                                                                  \
            hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                                    \
    } while (0)

// Which instantiation of the chunked kernels serves this geometry and these pointers.  Plain (gen = false): Hx and Nx whole numbers of
// 16-B chunks and every field 16-B aligned -- the geometry of the defaults, halo (4, 4, 4).  GEN (see the note in tpg_zipper_kernels.hpp)
// for everything else: an odd Hx (the reference's model halo (5, 5, 5)), 16-B-misaligned pointers, and -- with 8-B chunks, W = 2 --
// Float32 rows with Nx = 2 mod 4.  Nx is even (tripolar_grid.jl:81-83), so W = 2 always divides it: every geometry has a chunked form.
struct ChunkPlan { int W; bool gen; };
template <typename T>
ChunkPlan chunk_plan(const Geom& g, void* const fields[], int n)
{
    constexpr int WMAX = 16 / (int)sizeof(T);
    if (g.Hx % WMAX == 0 && g.Nx % WMAX == 0 && rows_on_16B_grid(0, fields, n)) return { WMAX, false };
    return { g.Nx % WMAX == 0 ? WMAX : 2, true };
}

// Kernel choice: column items (k_zipper_cols, plain or GEN: chunk_plan) for Hy <= 8; row items otherwise
// (k_zipper_vec for Hy > 8 -- e.g. the extended north halo of the split-explicit free surface -- on the plain geometry, k_zipper_scalar
// for Hy > 8 elsewhere and for Hy = 0).  TPG_ZIPPER_VARIANT=0 forces the row kernels everywhere (cross-check,
// tests/test_gpu_variants.py).  What was measured and dropped (tools/fillbench, profiles/r02/fillbench_ab.txt):
// plain loads (cold-dirty 26 vs 20 us), non-temporal stores (+2 us), write-through sc1 / sc0 sc1 buffer stores
// (-0.5 us cold-clean, +0 dirty), a persistent software-pipelined grid (1024 blocks, loads of item n+1 ahead of the
// stores of item n: -0.5 us), two half-row chunks per thread (one resident round of 4224 waves: +-0), 512 / 1024-thread
// blocks, two levels per thread (slower).  All of them, and same-shape pure copies, sit at 14.7-16.1 us cold:
// the 73 MB launch is at the copy ceiling of this access shape.
// COPY = true: the same-shape copy probe of the column kernel (tpg_testabi.hip), plain geometry only.
template <typename T, bool COPY = false>
int zipper_batch(void* const fields[], int n, const int8_t xloc[], const int8_t yloc[], const int32_t sign[],
                 const Geom& g, int kstart, int kcount, hipStream_t s)
{
    constexpr int WMAX = 16 / (int)sizeof(T);
    const ChunkPlan cp = chunk_plan<T>(g, fields, n);
    const bool vec = !cp.gen;                                        // the row-item kernel k_zipper_vec exists in the plain form only
    const bool cols = g.Hy >= 1 && g.Hy <= 8 && (COPY ? vec : tpg::config().zipper_variant != 0);    // Hy = 0: only the row-Ny substitution remains (row kernels)
    if (COPY && !cols) { tpg::set_error("copy probe: geometry has no plain column kernel"); return TPG_ERR_UNSUPPORTED; }
    FieldTable ft;
    const bool chunked = cols || vec;
    // nchunks; fix0 = first chunk / element (0-based) holding an i > Nx/2
    const ZipArgs a{ g.Nx, g.Ny, g.Hx, g.Hy, g.Hz, g.sx, g.plane, kstart, kcount, chunked ? g.Nx / cp.W : g.Nx, chunked ? (g.Nx / 2) / cp.W : g.Nx / 2 };
    fill_field_table(ft, fields, xloc, yloc, sign, n);
    long long total = 0;
    for (int f = 0; f < n; ++f) {
        ft.item0[f] = (int)total;
        long long per_level = cols ? a.nchunks
                                   : (long long)g.Hy * a.nchunks + (yloc[f] == TPG_CENTER ? a.nchunks - a.fix0 : 0);
        total += per_level * kcount;
        if (total >= (1ll << 31)) { tpg::set_error("zipper batch too large for 32-bit item index"); return TPG_ERR_UNSUPPORTED; }
    }
    ft.item0[n] = (int)total;
    if (total == 0) return TPG_OK;
    if (cols) {
        dim3 grid2((unsigned)(((long long)kcount * a.nchunks + 255) / 256), (unsigned)n);
        auto launch = [&](auto w, auto gen) {
            dispatch_hy(g.Hy, [&](auto hy) {
                TPG_LAUNCH((k_zipper_cols<T, decltype(w)::value, decltype(hy)::value, COPY, decltype(gen)::value>), grid2, dim3(256), s, ft, a);
            });
        };
        if constexpr (COPY) launch(std::integral_constant<int, WMAX>{}, std::false_type{});
        else dispatch_chunk<T>(cp.W, cp.gen, launch);
    } else {
        dim3 grid((unsigned)((total + 255) / 256));
        if (vec) TPG_LAUNCH((k_zipper_vec<T, WMAX>), grid, dim3(256), s, ft, a);
        else     TPG_LAUNCH((k_zipper_scalar<T>), grid, dim3(256), s, ft, a);
    }
    return tpg::launch_status("k_zipper");
}

// one batch of the merged fill (zipper with its corner cells + periodic x); 1 <= Hy <= 8
template <typename T>
int merged_batch(const FieldTable& t, const MergedArgs& a, int n, int Hy, ChunkPlan cp, hipStream_t s)
{
    const long long itemsB = a.rowsB * a.hw;
    dim3 grid(a.blocksA + a.blocksS + (unsigned)((itemsB + 255) / 256), (unsigned)n);
    dispatch_chunk<T>(cp.W, cp.gen, [&](auto w, auto gen) {
        dispatch_hy(Hy, [&](auto hy) {
            TPG_LAUNCH((k_fill_merged<T, decltype(w)::value, decltype(hy)::value, decltype(gen)::value>), grid, dim3(256), s, t, a);
        });
    });
    return tpg::launch_status("k_fill_merged");
}

// one batch of the fused small-field fill in its chunked form
template <typename T>
void fused_vec_launch(dim3 grid, hipStream_t s, const FieldTable& t, const FusedVecArgs& v, ChunkPlan cp)
{
    dispatch_chunk<T>(cp.W, cp.gen, [&](auto w, auto gen) {
        TPG_LAUNCH((k_fill_fused_vec<T, decltype(w)::value, decltype(gen)::value>), grid, dim3(256), s, t, v);
    });
}

}  // namespace
