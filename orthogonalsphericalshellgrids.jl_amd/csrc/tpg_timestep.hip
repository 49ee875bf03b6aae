// tpg_timestep.hip -- the head of a split-explicit hydrostatic step, for gfx950: the quasi-Adams-Bashforth-2 step of the velocities with the
// barotropic forcing of the free surface's sub-cycle (tpg_ab2_step_velocities) and of the tracers (tpg_ab2_step_fields).
// [recalled: Oceananigans' QuasiAdamsBashforth2 `ab2_step_velocities!`, `ab2_step_tracers!`, `store_tendencies!` and, for a split-explicit
// free surface, `_compute_integrated_ab2_tendencies!`; parity unpinned, like every operator here.]
//
// Fields
// - `u` at (Face, Center, Center), `v` at (Center, Face, Center), the tracers, and every tendency `Gn` (this step's) and `Gm` (the previous
//   step's): padded parents of ONE geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
// - `GU`, `GV`: 2-D padded planes of `(Ny + 2 Hy2) x (Nx + 2 Hx)`: the same `Hx`, so the same row pitch `sx` as the 3-D fields, and THEIR OWN
//   north / south halo `Hy2` (the free surface's fields live on the extended-halo grid).  First interior cell: `sx Hy2 + Hx`.
// - `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]` in the field type.  `n_fc`, `n_cf`: null, or Ny x Nx int32 count planes.
// The rule, for every interior node, in the field type T, in exactly this order, no contraction, every operation one correctly rounded IEEE
// operation (dt and chi converted to T once):
//     c1 = T(1.5) + chi_T          c2 = T(0.5) + chi_T          one addition each, formed once per call (on the host, in T)
//     g  = c1 * Gn[i,j,k] - c2 * Gm[i,j,k]                      EULER:  g = c1 * Gn[i,j,k], Gm is NOT read
//     x[i,j,k] = x[i,j,k] + dt_T * g
//     STORE:  Gm[i,j,k] = Gn[i,j,k]
// and, where GU is given, the forcing of the sub-cycle:
//     ĝ_k = +0 where k <= min(max(n_fc[i,j], 0), Nz), g otherwise
//     GU[i,j] = dz_c[1] * ĝ_1;     for k = 2..Nz:  GU[i,j] = GU[i,j] + dz_c[k] * ĝ_k
// - Only interior cells are written; no halo cell of any array is read.  There is no stencil: every halo width >= 0 is accepted.
// - The velocity itself is stepped with the unmasked g: its mask is the correction's (tpg_barotropic_correction), later in the step.
//
// Both are HBM-bound streams, one field per grid.y, ONE launch for all fields of a call.
// With an integral (k_ab2_velocities): a work item is ONE chunk of W interior columns and walks ALL levels with the running integral in
// registers -- level segments would re-associate the sum, which is not the rule.  Only the integral's add depends on the previous level; no
// load does: the loads of the next LOOKAHEAD levels of the three input streams (x, Gn, Gm) are issued before the current level's arithmetic
// (the ring of k_barotropic_mode, three vectors per level).  An item stores x, and Gm under STORE, at its own cells only: in place, no race.
// Without one (k_ab2_fields: the tracers, and the velocities when neither GU nor GV is given): nothing is carried from level to level, so an
// item is one chunk x a SEGMENT of consecutive levels, BATCH levels at a time, loads first, then arithmetic and stores.  Items are numbered
// (segment, row, chunk), chunk fastest.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over all
// the arrays passed (the 2-D planes share sx and Hx, so their interior sits on the 16-B grid exactly when their pointer does).  Element
// offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "../../include/tripolar_hip_timestep.h"

// compile-time switches of the A/B in profiles/ab2/ (make TIMESTEP_TAG=_la8 TIMESTEP_FLAGS='-DTPG_AB2_LOOKAHEAD=8', -DTPG_AB2_SEG=75,
// -DTPG_AB2_BATCH=2 or -DTPG_AB2_NT=0).  Measured at 3600 x 1800 x 75, one switch at a time from look-ahead 4, plain stores, 75 levels per
// item: streaming stores take 7 - 8 % off the velocity call and 2 % off the fields call; segments of 5 levels take 6 % off the fields call
// (segments of 16: 2 %); look-ahead 8 takes 8 % off the velocity call at 2 - 3 times the registers, look-ahead 2 adds 1 %, look-ahead 16
// takes 2.3 times as long.  With streaming stores look-ahead 8 is 0 - 2 % ahead of 4.  Look-ahead 4, streaming stores and segments of 5 are
// taken (profiles/ab2/).
#ifndef TPG_AB2_LOOKAHEAD
#define TPG_AB2_LOOKAHEAD 4
#endif
#ifndef TPG_AB2_SEG
#define TPG_AB2_SEG 5
#endif
#ifndef TPG_AB2_BATCH
#define TPG_AB2_BATCH 4
#endif
#ifndef TPG_AB2_NT
#define TPG_AB2_NT 1
#endif

namespace {

constexpr int LA = TPG_AB2_LOOKAHEAD;      // the velocities: levels whose loads are in flight ahead of the arithmetic
constexpr int SEG = TPG_AB2_SEG;           // the fields: levels per work item
constexpr int BATCH = TPG_AB2_BATCH;       // the fields: levels loaded before the first of them is stored
constexpr bool NT = TPG_AB2_NT;            // x and Gm go out in streaming (non-temporal) stores

struct Ab2Ptrs {
    void* x[TPG_MAX_FIELDS];               // the fields stepped (the velocities: u and / or v, packed to the front)
    const void* gn[TPG_MAX_FIELDS];        // this step's tendencies
    void* gm[TPG_MAX_FIELDS];              // the previous step's (null: EULER without STORE)
    void* G[2];                            // the velocities: GU / GV, or null
    const int32_t* n[2];                   // the velocities: n_fc / n_cf, or null
    const void* dz;
};

struct Ab2Args {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int rowitems;                          // Ny * cpr
    int items;                             // rowitems (walk-all), segments x rowitems (segmented)
    long long plane;                       // sx * sy
    long long off3;                        // the first interior cell of a 3-D parent
    long long off2;                        // sx * Hy2 + Hx: the first interior cell of a 2-D plane
    double c1, c2, dt;                     // T values held in doubles
};

// one level of the rule on a chunk: x <- x + dt g, g returned
template <typename T, int W, bool EULER, typename V>
__device__ __forceinline__ V ab2_level(V& x, const V gn, const V gm, T c1, T c2, T dt)
{
    V g;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        if constexpr (EULER) g[e] = c1 * gn[e];
        else g[e] = c1 * gn[e] - c2 * gm[e];
        x[e] = x[e] + dt * g[e];
    }
    return g;
}

template <typename T, int W, bool GEN, bool EULER, bool STORE>
__global__ __launch_bounds__(256) void k_ab2_velocities(Ab2Ptrs p, Ab2Args a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int j = item / a.cpr;                                    // interior row (0-based)
    const int e0 = (item - j * a.cpr) * W;                         // first interior column of the chunk (0-based)
    const long long row = (long long)a.sx * j + e0;
    const int f = blockIdx.y;
    T* x = static_cast<T*>(p.x[f]) + a.off3 + row;
    const T* gn = static_cast<const T*>(p.gn[f]) + a.off3 + row;
    T* gm = (!EULER || STORE) ? static_cast<T*>(p.gm[f]) + a.off3 + row : nullptr;
    T* G = static_cast<T*>(p.G[f]);                                // one field of the two may have no integral
    const T* dz = static_cast<const T*>(p.dz);
    const T c1 = (T)a.c1, c2 = (T)a.c2, dt = (T)a.dt;

    int m[W];                                                      // masked levels of the integral (0-based k < m)
#pragma unroll
    for (int e = 0; e < W; ++e) m[e] = 0;
    if (G && p.n[f]) {
        const Counts<W> n = *reinterpret_cast<const Counts<W>*>(p.n[f] + (long long)a.Nx * j + e0);
#pragma unroll
        for (int e = 0; e < W; ++e) m[e] = min(max(n[e], 0), a.Nz);
    }

    cvec_t rx[LA], rn[LA], rm[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) {
        const long long o = a.plane * min(s, a.Nz - 1);
        rx[s] = *reinterpret_cast<const cvec_t*>(x + o);
        rn[s] = *reinterpret_cast<const cvec_t*>(gn + o);
        if constexpr (!EULER) rm[s] = *reinterpret_cast<const cvec_t*>(gm + o);
    }
    cvec_t acc;
    for (int k0 = 0; k0 < a.Nz; k0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int k = k0 + s;
            if (k >= a.Nz) break;
            cvec_t xv = rx[s];
            const cvec_t nv = rn[s];
            cvec_t mv = nv;
            if constexpr (!EULER) mv = rm[s];
            if (k + LA < a.Nz) {                                   // level k + LA goes out before level k's arithmetic
                const long long o = a.plane * (k + LA);
                rx[s] = *reinterpret_cast<const cvec_t*>(x + o);
                rn[s] = *reinterpret_cast<const cvec_t*>(gn + o);
                if constexpr (!EULER) rm[s] = *reinterpret_cast<const cvec_t*>(gm + o);
            }
            const cvec_t g = ab2_level<T, W, EULER>(xv, nv, mv, c1, c2, dt);
            const long long o = a.plane * k;
            store_chunk<NT>(reinterpret_cast<cvec_t*>(x + o), xv);
            if constexpr (STORE) store_chunk<NT>(reinterpret_cast<cvec_t*>(gm + o), nv);
            if (G) {
                const T d = dz[k];
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const T gh = k < m[e] ? T(0) : g[e];
                    if (k == 0) acc[e] = d * gh;                   // the first term is the product itself: +0 + (-0) would lose its sign
                    else acc[e] = acc[e] + d * gh;
                }
            }
        }
    }
    if (G) *reinterpret_cast<cvec_t*>(G + a.off2 + row) = acc;
}

template <typename T, int W, bool GEN, bool EULER, bool STORE>
__global__ __launch_bounds__(256) void k_ab2_fields(Ab2Ptrs p, Ab2Args a)
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
    const int f = blockIdx.y;
    T* x = static_cast<T*>(p.x[f]) + a.off3 + row;
    const T* gn = static_cast<const T*>(p.gn[f]) + a.off3 + row;
    T* gm = (!EULER || STORE) ? static_cast<T*>(p.gm[f]) + a.off3 + row : nullptr;
    const T c1 = (T)a.c1, c2 = (T)a.c2, dt = (T)a.dt;

    for (int kb = k0; kb < k1; kb += BATCH) {
        cvec_t xv[BATCH], nv[BATCH], mv[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            const long long o = a.plane * min(kb + b, k1 - 1);
            xv[b] = *reinterpret_cast<const cvec_t*>(x + o);
            nv[b] = *reinterpret_cast<const cvec_t*>(gn + o);
            if constexpr (!EULER) mv[b] = *reinterpret_cast<const cvec_t*>(gm + o);
            else mv[b] = nv[b];
        }
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            const int k = kb + b;
            if (k >= k1) break;
            ab2_level<T, W, EULER>(xv[b], nv[b], mv[b], c1, c2, dt);
            const long long o = a.plane * k;
            store_chunk<NT>(reinterpret_cast<cvec_t*>(x + o), xv[b]);
            if constexpr (STORE) store_chunk<NT>(reinterpret_cast<cvec_t*>(gm + o), nv[b]);
        }
    }
}

// the checks both calls start with, in this order
int check_shape(int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int Hy2, int ft, int flags)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (Hy2 < 0) { tpg::set_error("invalid north/south halo Hy2=%d of the 2-D planes", Hy2); return TPG_ERR_INVALID_ARGUMENT; }
    if (flags & ~(TPG_AB2_EULER | TPG_AB2_STORE_PREVIOUS)) {
        tpg::set_error("unknown flag bits 0x%x (TPG_AB2_EULER | TPG_AB2_STORE_PREVIOUS are defined)", (unsigned)flags & ~(unsigned)(TPG_AB2_EULER | TPG_AB2_STORE_PREVIOUS));
        return TPG_ERR_INVALID_ARGUMENT;
    }
    return TPG_OK;
}

// T values in doubles: c1 = T(1.5) + chi_T, c2 = T(0.5) + chi_T, dt_T
template <typename T>
void ab2_constants(Ab2Args& a, double dt, double chi)
{
    const T chi_t = (T)chi;
    const T c1 = T(1.5) + chi_t, c2 = T(0.5) + chi_t;
    a.c1 = (double)c1;
    a.c2 = (double)c2;
    a.dt = (double)(T)dt;
}

// the segmented kernel over the nf fields packed in p; `arrays`: every array whose chunks it touches
int launch_fields(const Ab2Ptrs& p, int nf, void* const arrays[], int na, const Geom& g, double dt, double chi, int flags, int ft, hipStream_t st)
{
    const long long segs = (g.Nz + SEG - 1) / SEG;
    const bool euler = flags & TPG_AB2_EULER, store = flags & TPG_AB2_STORE_PREVIOUS;
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = g.Nx / cp.W;
        Ab2Args a{ g.Nx, g.Ny, g.Nz, g.sx, cpr, g.Ny * cpr, (int)(segs * g.Ny * cpr), g.plane, interior3(g), 0, 0.0, 0.0, 0.0 };
        ab2_constants<T>(a, dt, chi);
        dim3 grid((unsigned)((a.items + 255) / 256), (unsigned)nf);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            if (euler && store)  hipLaunchKernelGGL((k_ab2_fields<T, W, GEN, true, true>), grid, dim3(256), 0, st, p, a);
            else if (euler)      hipLaunchKernelGGL((k_ab2_fields<T, W, GEN, true, false>), grid, dim3(256), 0, st, p, a);
            else if (store)      hipLaunchKernelGGL((k_ab2_fields<T, W, GEN, false, true>), grid, dim3(256), 0, st, p, a);
            else                 hipLaunchKernelGGL((k_ab2_fields<T, W, GEN, false, false>), grid, dim3(256), 0, st, p, a);
        });
        return tpg::launch_status("k_ab2_fields");
    });
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_timestep_last_error(void) { return tpg_last_error(); }

int tpg_ab2_step_velocities(void* u, void* v, const void* Gu_n, const void* Gv_n, void* Gu_m, void* Gv_m, void* GU, void* GV, const void* dz_c,
                            const int32_t* n_fc, const int32_t* n_cf, double dt, double chi, int flags, int Nx, int Ny, int Nz, int Hx, int Hy,
                            int Hz, int Hy2, int ft, void* stream)
{
    if (int rc = check_shape(Nx, Ny, Nz, Hx, Hy, Hz, Hy2, ft, flags)) return rc;
    const bool euler = flags & TPG_AB2_EULER, store = flags & TPG_AB2_STORE_PREVIOUS;
    const bool need_m = !euler || store;
    if (!u && !v) {
        if (Gu_n || Gv_n || Gu_m || Gv_m || GU || GV) tpg::set_error("a tendency or a forcing plane given without its field: u and v both null");
        else tpg::set_error("u, v, their tendencies, GU and GV all null: nothing to compute");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if (!u != !Gu_n) { tpg::set_error("u and Gu_n must be given together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!v != !Gv_n) { tpg::set_error("v and Gv_n must be given together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!u && (Gu_m || GU)) { tpg::set_error("Gu_m or GU given without u: the group (u, Gu_n, Gu_m, GU) is null together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!v && (Gv_m || GV)) { tpg::set_error("Gv_m or GV given without v: the group (v, Gv_n, Gv_m, GV) is null together"); return TPG_ERR_INVALID_ARGUMENT; }
    if (u && !Gu_m && need_m) { tpg::set_error("null Gu_m: it may be null only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear"); return TPG_ERR_INVALID_ARGUMENT; }
    if (v && !Gv_m && need_m) { tpg::set_error("null Gv_m: it may be null only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear"); return TPG_ERR_INVALID_ARGUMENT; }
    if ((GU || GV) && !dz_c) { tpg::set_error("null dz_c with GU or GV given"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz;                    // the 3-D parents
    const unsigned long long pbytes = (unsigned long long)g.sx * (Ny + 2ll * Hy2) * esz;                   // GU, GV
    const unsigned long long cbytes = (unsigned long long)Nx * Ny * 4;                                     // the count planes
    const Span spans[11] = { { u, bytes, "u", true }, { v, bytes, "v", true }, { Gu_n, bytes, "Gu_n", false }, { Gv_n, bytes, "Gv_n", false },
                             { Gu_m, bytes, "Gu_m", store }, { Gv_m, bytes, "Gv_m", store }, { GU, pbytes, "GU", true }, { GV, pbytes, "GV", true },
                             { dz_c, (unsigned long long)Nz * esz, "dz_c", false }, { n_fc, cbytes, "n_fc", false }, { n_cf, cbytes, "n_cf", false } };
    for (int q = 0; q < 9; ++q)
        if (misaligned(esz, spans[q].p)) { tpg::set_error("%s pointer not aligned to its element type", spans[q].name); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(4, n_fc, n_cf)) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_overlaps(spans, 11, "an item writes its own cells while other items read theirs")) return rc;
    const bool integral = GU || GV;
    const long long segs = integral ? 1 : (Nz + SEG - 1) / SEG;
    if (segs * Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("ab2 velocity step: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    Ab2Ptrs p{};
    void* arrays[8];
    int nf = 0, na = 0;
    auto add = [&](void* x, const void* gn, void* gm, void* G, const int32_t* n) {
        p.x[nf] = x; p.gn[nf] = gn; p.gm[nf] = need_m ? gm : nullptr; p.G[nf] = G; p.n[nf++] = n;
        arrays[na++] = x; arrays[na++] = const_cast<void*>(gn);
        if (need_m) arrays[na++] = gm;
        if (G) arrays[na++] = G;
    };
    if (u) add(u, Gu_n, Gu_m, GU, n_fc);
    if (v) add(v, Gv_n, Gv_m, GV, n_cf);
    p.dz = dz_c;
    hipStream_t st = tpg::as_stream(stream);
    if (!integral) return launch_fields(p, nf, arrays, na, g, dt, chi, flags, ft, st);     // nothing carried from level to level: segments
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        Ab2Args a{ Nx, Ny, Nz, g.sx, cpr, Ny * cpr, Ny * cpr, g.plane, interior3(g), (long long)g.sx * Hy2 + Hx, 0.0, 0.0, 0.0 };
        ab2_constants<T>(a, dt, chi);
        dim3 grid((unsigned)((a.items + 255) / 256), (unsigned)nf);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            if (euler && store)  hipLaunchKernelGGL((k_ab2_velocities<T, W, GEN, true, true>), grid, dim3(256), 0, st, p, a);
            else if (euler)      hipLaunchKernelGGL((k_ab2_velocities<T, W, GEN, true, false>), grid, dim3(256), 0, st, p, a);
            else if (store)      hipLaunchKernelGGL((k_ab2_velocities<T, W, GEN, false, true>), grid, dim3(256), 0, st, p, a);
            else                 hipLaunchKernelGGL((k_ab2_velocities<T, W, GEN, false, false>), grid, dim3(256), 0, st, p, a);
        });
        return tpg::launch_status("k_ab2_velocities");
    });
}

int tpg_ab2_step_fields(void* const fields[], const void* const Gn[], void* const Gm[], int n, double dt, double chi, int flags, int Nx, int Ny,
                        int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = check_shape(Nx, Ny, Nz, Hx, Hy, Hz, 0, ft, flags)) return rc;
    const bool euler = flags & TPG_AB2_EULER, store = flags & TPG_AB2_STORE_PREVIOUS;
    const bool need_m = !euler || store;
    if (!fields || !Gn || n < 1) { tpg::set_error("no fields"); return TPG_ERR_INVALID_ARGUMENT; }
    if (n > TPG_MAX_FIELDS) { tpg::set_error("%d fields: at most TPG_MAX_FIELDS = %d in one call", n, TPG_MAX_FIELDS); return TPG_ERR_INVALID_ARGUMENT; }
    if (!Gm && need_m) { tpg::set_error("null Gm table: it may be null only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear"); return TPG_ERR_INVALID_ARGUMENT; }
    for (int f = 0; f < n; ++f) {
        if (!fields[f]) { tpg::set_error("null field %d", f); return TPG_ERR_INVALID_ARGUMENT; }
        if (!Gn[f]) { tpg::set_error("null Gn of field %d", f); return TPG_ERR_INVALID_ARGUMENT; }
        if (need_m && !Gm[f]) {
            tpg::set_error("null Gm of field %d: it may be null only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear", f);
            return TPG_ERR_INVALID_ARGUMENT;
        }
    }
    const size_t esz = elem_size(ft);
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz;
    Span spans[3 * TPG_MAX_FIELDS];
    int ns = 0;
    for (int f = 0; f < n; ++f) {
        Span* s = spans + ns;
        s[0] = Span{ fields[f], bytes, "", true };
        s[1] = Span{ Gn[f], bytes, "", false };
        s[2] = Span{ Gm ? Gm[f] : nullptr, bytes, "", store };
        snprintf(s[0].name, sizeof s[0].name, "field %d", f);
        snprintf(s[1].name, sizeof s[1].name, "Gn of field %d", f);
        snprintf(s[2].name, sizeof s[2].name, "Gm of field %d", f);
        ns += 3;
    }
    for (int q = 0; q < ns; ++q)
        if (misaligned(esz, spans[q].p)) { tpg::set_error("%s: pointer not aligned to its element type", spans[q].name); return TPG_ERR_INVALID_ARGUMENT; }
    if (int rc = check_overlaps(spans, ns, "an item writes its own cells while other items read theirs")) return rc;
    const long long segs = (Nz + SEG - 1) / SEG;
    if (segs * Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("ab2 field step: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    Ab2Ptrs p{};
    void* arrays[3 * TPG_MAX_FIELDS];
    int na = 0;
    for (int f = 0; f < n; ++f) {
        p.x[f] = fields[f]; p.gn[f] = Gn[f]; p.gm[f] = need_m ? Gm[f] : nullptr;
        arrays[na++] = fields[f]; arrays[na++] = const_cast<void*>(Gn[f]);
        if (need_m) arrays[na++] = Gm[f];
    }
    return launch_fields(p, n, arrays, na, g, dt, chi, flags, ft, tpg::as_stream(stream));
}

}  // extern "C"
