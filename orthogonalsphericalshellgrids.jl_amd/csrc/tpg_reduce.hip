// tpg_reduce.hip -- device reductions for gfx950: field extrema (tpg_field_extrema) and the advective CFL timescale
// (tpg_cell_advection_timescale), with their workspace bound (tpg_reduce_workspace_bytes).
//
// What a model driver runs between steps: maximum(u), maximum(v) in the progress callback, TimeStepWizard's cell_advection_timescale
// (examples/bickley_jet.jl:75,84,87), and the six metric reductions of a grid's `show`.  Min and max only: exact and independent of order,
// so the results are bit-reproducible and compare bit for bit with a host reference.
//
// HBM-bound reads.  A block owns interior rows (row r = k * Ny + j, grid-stride over blocks: consecutive blocks stream consecutive rows);
// its threads stride over the row's chunks of W interior columns -- 16-B loads where rows and pointers sit on the 16-B grid, the same
// chunks loaded element-aligned otherwise (odd Hx, Float32 rows with Nx = 2 mod 4 in 8-B chunks, offset pointers): chunk_plan's plain /
// GEN split.  Row and level are block-uniform (scalar address arithmetic, one scalar load of dz_f[k]); no index division per element.
// Per-lane accumulators (min, max, a NaN flag) -> wave64 shuffle -> across the four waves through LDS -> ONE partial per block into the
// workspace -> a second, tiny launch reduces the partials and writes `out`.  No float atomics, no inter-block flag or counter, no
// dependence on dispatch order: nothing waits on another block, and the extra launch boundary is microseconds against milliseconds.
//
// NaN: comparisons drop a NaN operand, so each lane keeps a flag (x != x) beside its accumulators and turns them into NaN before the
// cross-lane steps, whose min / max PROPAGATE a NaN operand (Julia's minimum / maximum, not fmin).  max |c| = max(-min c, max c) is formed
// once, in the final launch.  The timescale reduces max s and divides once: correctly rounded division is monotone (s >= 0), so
// 1 / max s == min (1 / s) bit for bit; -ffp-contract=off and hipcc's correctly rounded Float32 division (its default) keep s itself exact.
#include "tpg_launch.hpp"

namespace {

constexpr int RB = 256;                    // threads per block: four waves
constexpr int RED_MAX_BLOCKS = 2048;       // 256 CUs x 8 resident blocks; the rows beyond are the grid-stride loop's

struct ExtremaTable {
    const void* ptr[TPG_MAX_FIELDS];
    const int32_t* counts[TPG_MAX_FIELDS];
    int zloc[TPG_MAX_FIELDS];
};

struct TauPtrs {
    const void *u, *v, *w, *dx, *dy, *dz;
    const int32_t* ncc;
};

struct RedArgs {
    int Nx, Ny, Nz, Hx, Hy, Hz, sx;
    int cpr;                               // chunks per interior row
    long long plane;                       // sx * sy
};

template <int W> struct CountVec { typedef int type __attribute__((ext_vector_type(W), aligned(4))); };

__device__ inline double tabs(double x) { return __builtin_fabs(x); }
__device__ inline float tabs(float x) { return __builtin_fabsf(x); }

// min / max that PROPAGATE a NaN operand
__device__ inline double pmin(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ inline double pmax(double a, double b) { return (b > a || b != b) ? b : a; }

// (mn, mx) of the block in thread 0; `s` is the block's one LDS object, 2 * RB / 64 doubles
__device__ inline void block_min_max(double& mn, double& mx, double* s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = pmin(mn, __shfl_xor(mn, o));
        mx = pmax(mx, __shfl_xor(mx, o));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s[2 * wave] = mn; s[2 * wave + 1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < RB / 64; ++w) { mn = pmin(mn, s[2 * w]); mx = pmax(mx, s[2 * w + 1]); }
}

template <typename T, int W, bool GEN>
__global__ __launch_bounds__(RB) void k_field_extrema(ExtremaTable t, RedArgs a, double* __restrict__ partial)
{
    typedef typename Vec<T, W>::aligned_t vec_t;
    typedef typename Vec<T, W>::loose_t lvec_t;
    typedef typename std::conditional<GEN, lvec_t, vec_t>::type cvec_t;
    __shared__ double lds[2 * RB / 64];
    const int f = blockIdx.y;                                      // block-uniform: table reads are scalar loads
    const T* base = static_cast<const T*>(t.ptr[f]) + a.plane * a.Hz + (long long)a.sx * a.Hy + a.Hx;
    const int32_t* cnt = t.counts[f];
    const int zl = cnt ? t.zloc[f] : 0;
    const int top = a.Nz - zl;                                     // a z-Face field's last level is never left out
    const int rows = a.Ny * a.Nz;
    T mn = (T)INFINITY, mx = -(T)INFINITY;
    bool bad = false;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const int k = r / a.Ny, j = r - k * a.Ny;                  // 0-based level and row
        const T* row = base + a.plane * k + (long long)a.sx * j;
        if (!cnt) {
#pragma unroll 4
            for (int c = threadIdx.x; c < a.cpr; c += RB) {
                const cvec_t v = *reinterpret_cast<const cvec_t*>(row + c * W);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const T x = v[e];
                    mn = x < mn ? x : mn;
                    mx = x > mx ? x : mx;
                    bad |= x != x;
                }
            }
        } else {
            const int32_t* crow = cnt + (long long)a.Nx * j;
            for (int c = threadIdx.x; c < a.cpr; c += RB) {
                const typename CountVec<W>::type n = *reinterpret_cast<const typename CountVec<W>::type*>(crow + c * W);
                bool in[W], any = false;                           // counted: above the masked levels k < min(n + zl, top) of its column
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    in[e] = k >= min(n[e] + zl, top);
                    any |= in[e];
                }
                if (!any) continue;                                // a chunk of masked cells is not read
                const cvec_t v = *reinterpret_cast<const cvec_t*>(row + c * W);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const T x = v[e];
                    if (in[e]) {
                        mn = x < mn ? x : mn;
                        mx = x > mx ? x : mx;
                        bad |= x != x;
                    }
                }
            }
        }
    }
    double dmn = bad ? (double)NAN : (double)mn, dmx = bad ? (double)NAN : (double)mx;
    block_min_max(dmn, dmx, lds);
    if (threadIdx.x == 0) {
        double* p = partial + 2 * ((long long)f * gridDim.x + blockIdx.x);
        p[0] = dmn;
        p[1] = dmx;
    }
}

// one block per field: the nb partials of the field -> out[3f .. 3f+2]
__global__ __launch_bounds__(RB) void k_field_extrema_final(const double* __restrict__ partial, int nb, double* __restrict__ out)
{
    __shared__ double lds[2 * RB / 64];
    const int f = blockIdx.x;
    const double* p = partial + 2 * (long long)f * nb;
    double mn = (double)INFINITY, mx = -(double)INFINITY;
    for (int b = threadIdx.x; b < nb; b += RB) {
        mn = pmin(mn, p[2 * b]);
        mx = pmax(mx, p[2 * b + 1]);
    }
    block_min_max(mn, mx, lds);
    if (threadIdx.x == 0) {
        out[3 * f] = mn;
        out[3 * f + 1] = mx;
        out[3 * f + 2] = pmax(-mn, mx);                            // max |c|; -Inf for an empty set, NaN with the other two
    }
}

template <typename T, int W, bool GEN>
__global__ __launch_bounds__(RB) void k_advection_smax(TauPtrs p, RedArgs a, double* __restrict__ partial)
{
    typedef typename Vec<T, W>::aligned_t vec_t;
    typedef typename Vec<T, W>::loose_t lvec_t;
    typedef typename std::conditional<GEN, lvec_t, vec_t>::type cvec_t;
    __shared__ double lds[2 * RB / 64];
    const long long off2 = (long long)a.sx * a.Hy + a.Hx, off3 = a.plane * a.Hz + off2;
    const T* u = static_cast<const T*>(p.u) + off3;
    const T* v = static_cast<const T*>(p.v) + off3;
    const T* w = static_cast<const T*>(p.w) + off3;                // w's levels 1..Nz: its level Nz + 1 is not read
    const T* dx = static_cast<const T*>(p.dx) + off2;
    const T* dy = static_cast<const T*>(p.dy) + off2;
    const T* dz = static_cast<const T*>(p.dz);
    const int rows = a.Ny * a.Nz;
    T smax = 0;                                                    // s >= 0: the maximum over no cell at all is 0, tau = +Inf
    bool bad = false;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const int k = r / a.Ny, j = r - k * a.Ny;
        const long long o2 = (long long)a.sx * j, o3 = a.plane * k + o2;
        const T dzk = dz[k];
        const int32_t* crow = p.ncc ? p.ncc + (long long)a.Nx * j : nullptr;
#pragma unroll 2
        for (int c = threadIdx.x; c < a.cpr; c += RB) {
            bool in[W], any = false;
            if (crow) {
                const typename CountVec<W>::type n = *reinterpret_cast<const typename CountVec<W>::type*>(crow + c * W);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    in[e] = k >= n[e];                             // cells k <= n_cc (1-based) are left out
                    any |= in[e];
                }
                if (!any) continue;
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) in[e] = true;
            }
            const cvec_t uu = *reinterpret_cast<const cvec_t*>(u + o3 + c * W);
            const cvec_t vv = *reinterpret_cast<const cvec_t*>(v + o3 + c * W);
            const cvec_t ww = *reinterpret_cast<const cvec_t*>(w + o3 + c * W);
            const cvec_t ddx = *reinterpret_cast<const cvec_t*>(dx + o2 + c * W);
            const cvec_t ddy = *reinterpret_cast<const cvec_t*>(dy + o2 + c * W);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const T s = tabs(uu[e]) / ddx[e] + tabs(vv[e]) / ddy[e] + tabs(ww[e]) / dzk;      // left to right, in T
                if (in[e]) {
                    smax = s > smax ? s : smax;
                    bad |= s != s;
                }
            }
        }
    }
    double dmx = bad ? (double)NAN : (double)smax, unused = dmx;
    block_min_max(unused, dmx, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = dmx;
}

template <typename T>
__global__ __launch_bounds__(RB) void k_advection_final(const double* __restrict__ partial, int nb, double* __restrict__ out)
{
    __shared__ double lds[2 * RB / 64];
    double mx = 0, unused = 0;
    for (int b = threadIdx.x; b < nb; b += RB) mx = pmax(mx, partial[b]);
    block_min_max(unused, mx, lds);
    if (threadIdx.x == 0) out[0] = (double)((T)1 / (T)mx);         // the partials are T values held in doubles; 1 / 0 = +Inf, 1 / NaN = NaN
}

int red_blocks(int Ny, int Nz)
{
    const long long rows = (long long)Ny * Nz;
    return (int)(rows < RED_MAX_BLOCKS ? rows : RED_MAX_BLOCKS);
}

// rows are indexed by an int that the grid-stride loop advances by at most RED_MAX_BLOCKS past the last row
int check_rows(int Ny, int Nz)
{
    if ((long long)Ny * Nz >= (1ll << 31) - 2 * RED_MAX_BLOCKS) {
        tpg::set_error("reduction: %lld interior rows are too many for 32-bit work-item indexing", (long long)Ny * Nz);
        return TPG_ERR_UNSUPPORTED;
    }
    return TPG_OK;
}

int check_out_and_workspace(const double* out, const void* workspace, size_t workspace_bytes, size_t need)
{
    if (!out) { tpg::set_error("null out"); return TPG_ERR_INVALID_ARGUMENT; }
    if ((uintptr_t)out % 8) { tpg::set_error("out pointer not aligned to double"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!workspace) { tpg::set_error("null workspace (%zu bytes needed: tpg_reduce_workspace_bytes)", need); return TPG_ERR_WORKSPACE; }
    if ((uintptr_t)workspace % 8) { tpg::set_error("workspace not 8-B aligned"); return TPG_ERR_WORKSPACE; }
    if (workspace_bytes < need) { tpg::set_error("workspace too small: %zu bytes given, %zu needed", workspace_bytes, need); return TPG_ERR_WORKSPACE; }
    return TPG_OK;
}

}  // namespace

extern "C" {

size_t tpg_reduce_workspace_bytes(int nfields, int Nx, int Ny, int Nz)
{
    (void)Nx;                                                      // one partial per block, and blocks own rows
    const long long rows = (long long)(Ny < 1 ? 1 : Ny) * (Nz < 1 ? 1 : Nz);
    const size_t blocks = (size_t)(rows < RED_MAX_BLOCKS ? rows : RED_MAX_BLOCKS);
    return (size_t)(nfields < 1 ? 1 : nfields) * blocks * 2 * sizeof(double);
}

int tpg_field_extrema(void* const fields[], int nfields, const int32_t* const counts[], const int8_t zloc[], double* out, void* workspace,
                      size_t workspace_bytes, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc) return rc;
    if (counts && !zloc) { tpg::set_error("a counts table needs a zloc table"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    for (int f = 0; f < nfields; ++f) {
        if ((uintptr_t)fields[f] % esz) { tpg::set_error("field %d: pointer not aligned to its element type", f); return TPG_ERR_INVALID_ARGUMENT; }
        if (!counts || !counts[f]) continue;
        if (zloc[f] != TPG_CENTER && zloc[f] != TPG_FACE) { tpg::set_error("field %d: zloc = %d is neither TPG_CENTER nor TPG_FACE", f, (int)zloc[f]); return TPG_ERR_INVALID_ARGUMENT; }
        if ((uintptr_t)counts[f] % 4) { tpg::set_error("field %d: count plane pointer not aligned to int32", f); return TPG_ERR_INVALID_ARGUMENT; }
    }
    if ((rc = check_rows(Ny, Nz))) return rc;
    const int nb = red_blocks(Ny, Nz);
    if ((rc = check_out_and_workspace(out, workspace, workspace_bytes, (size_t)nfields * nb * 2 * sizeof(double)))) return rc;
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    hipStream_t st = tpg::as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    rc = for_each_batch(nfields, [&](int f0, int n) {
        ExtremaTable t;
        for (int f = 0; f < n; ++f) {
            t.ptr[f] = fields[f0 + f];
            t.counts[f] = counts ? counts[f0 + f] : nullptr;
            t.zloc[f] = t.counts[f] ? zloc[f0 + f] : 0;
        }
        return dispatch_ft(ft, [&](auto ty) {
            typedef decltype(ty) T;
            const ChunkPlan cp = chunk_plan<T>(g, fields + f0, n);
            const RedArgs a{ Nx, Ny, Nz, Hx, Hy, Hz, g.sx, Nx / cp.W, g.plane };
            dispatch_chunk<T>(cp.W, cp.gen, [&](auto w, auto gen) {
                hipLaunchKernelGGL((k_field_extrema<T, decltype(w)::value, decltype(gen)::value>), dim3((unsigned)nb, (unsigned)n), dim3(RB), 0, st,
                                   t, a, partial + 2 * (size_t)f0 * nb);
            });
            return tpg::launch_status("k_field_extrema");
        });
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_field_extrema_final, dim3((unsigned)nfields), dim3(RB), 0, st, partial, nb, out);
    return tpg::launch_status("k_field_extrema_final");
}

int tpg_cell_advection_timescale(const void* u, const void* v, const void* w, const void* dx_fc, const void* dy_cf, const void* dz_f,
                                 const int32_t* n_cc, double* out, void* workspace, size_t workspace_bytes,
                                 int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc) return rc;
    if (!u || !v || !w) { tpg::set_error("null u, v or w"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!dx_fc || !dy_cf || !dz_f) { tpg::set_error("null dx_fc, dy_cf or dz_f"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    if (((uintptr_t)u | (uintptr_t)v | (uintptr_t)w) % esz) { tpg::set_error("u, v or w pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    if (((uintptr_t)dx_fc | (uintptr_t)dy_cf | (uintptr_t)dz_f) % esz) {
        tpg::set_error("dx_fc, dy_cf or dz_f pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if ((uintptr_t)n_cc % 4) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    if ((rc = check_rows(Ny, Nz))) return rc;
    const int nb = red_blocks(Ny, Nz);
    if ((rc = check_out_and_workspace(out, workspace, workspace_bytes, (size_t)nb * sizeof(double)))) return rc;
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    hipStream_t st = tpg::as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    const TauPtrs p{ u, v, w, dx_fc, dy_cf, dz_f, n_cc };
    void* const arrays[5] = { const_cast<void*>(u), const_cast<void*>(v), const_cast<void*>(w), const_cast<void*>(dx_fc), const_cast<void*>(dy_cf) };
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, 5);
        const RedArgs a{ Nx, Ny, Nz, Hx, Hy, Hz, g.sx, Nx / cp.W, g.plane };
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto wd, auto gen) {
            hipLaunchKernelGGL((k_advection_smax<T, decltype(wd)::value, decltype(gen)::value>), dim3((unsigned)nb), dim3(RB), 0, st, p, a, partial);
        });
        if (int e = tpg::launch_status("k_advection_smax")) return e;
        hipLaunchKernelGGL((k_advection_final<T>), dim3(1), dim3(RB), 0, st, partial, nb, out);
        return tpg::launch_status("k_advection_final");
    });
}

}  // extern "C"
