// tpg_vertical_diffusion.hip -- the vertically implicit diffusion step of a hydrostatic model for gfx950 (tpg_vertical_implicit_diffusion):
// a batched tridiagonal solve along z, one matrix per column and up to TPG_MAX_FIELDS right-hand sides per call, in place; what Oceananigans'
// implicit_step! does to u, v and every tracer right after their AB2 update under a VerticallyImplicitTimeDiscretization closure.
// [recalled: Oceananigans' ivd_upper_diagonal / ivd_lower_diagonal / ivd_diagonal, kappa_dz2, and solve_batched_tridiagonal_system_z!; parity
// unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_vertical_diffusion.h.  Evaluated in the field type T with no contraction; every
// operation is one correctly rounded IEEE operation.  No halo cell is read or written.
//
// ONE launch, of the family of k_w_from_continuity (tpg_continuity.hip) and k_ab2_velocities (tpg_timestep.hip): a work item is ONE chunk of W
// interior columns of one row.  It walks ALL levels twice.  Upwards it forms up, lo, diag, t and beta ONCE per level for all n fields (four
// divisions for the coefficients and one for t), then one division per field: the forward phi goes to the field's own cell in an ordinary
// store, t[k] to the storage policy.  Downwards it reads phi[k] back from the field and t[k+1] from the policy and stores the result.  Both
// walks keep the loads of the next LA levels in flight (a ring of register slots): no load depends on the previous level, only the carried
// beta, up and phi do.  The item re-reads only what it wrote itself, so nothing is synchronised.
// The two storage policies of t (ONCHIP): LDS laid out [level][lane], 16 B per lane, so a wave's lanes hit consecutive banks and a lane only
// ever touches its own slot (blocks of one wave, no barrier); or `scratch`, a padded parent, at the cell's own offset.  Everything else is the
// same code, so the same bits.
// The fields of a call are a compile-time bound NF in {1, 2, 4, 16} with the run-time n <= NF inside it (wave-uniform predicates): the
// carried phi of every field stays in registers.  kappa is a chunk per level (FIELD) or a wave-uniform value (a profile entry or the
// constant).  The mask is a run-time flag: without counts every column starts at level 0.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over the
// fields, scratch and a FIELD kappa.  Element offsets are 64-bit.  No atomics, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "../../include/tripolar_hip_vertical_diffusion.h"
#include <cmath>
#include <limits>

// compile-time switch of the A/B in profiles/vertical_diffusion/ (make VERTICAL_DIFFUSION_TAG=_nt0 VERTICAL_DIFFUSION_FLAGS=-DTPG_VDIFF_NT=0):
// the final stores of the back sweep as streaming stores.  Measured at 3600 x 1800 x 75 on a rotating-order run: 10 % (Float64) and 8 %
// (Float32) off the streamed call, disjoint ranges; overlapping ranges on the on-chip path.  Taken.  The forward stores are
// re-read and stay cacheable in every build.
#ifndef TPG_VDIFF_NT
#define TPG_VDIFF_NT 1
#endif

namespace {

constexpr bool NT = TPG_VDIFF_NT;
constexpr int ON_CHIP_LANES = 64;                      // the on-chip path: blocks of one wave
constexpr int LDS_BYTES = 160 * 1024;                  // per CU, and per block, on gfx950
constexpr int ON_CHIP_LEVELS = LDS_BYTES / (ON_CHIP_LANES * 16);      // 16 B of t per lane and level: 160 levels

// levels whose loads are in flight ahead of the arithmetic, by the fields in registers
template <int NF> constexpr int LOOKAHEAD = NF <= 2 ? 4 : NF <= 4 ? 2 : 1;

struct VdiffPtrs {
    void* x[TPG_MAX_FIELDS];               // the fields, solved in place
    const void* kappa;                     // PROFILE: Nz + 1 values; FIELD: a padded parent; CONSTANT: null
    const void* dzc;                       // Nz values
    const void* dzf;                       // Nz + 1 values
    const int32_t* counts;                 // null, or an Ny x Nx plane
    void* t;                               // the streamed path: scratch
};

struct VdiffArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int items;                             // Ny * cpr
    int n;                                 // fields of the call
    int profile;                           // kappa is a table (not FIELD, not CONSTANT)
    long long plane;                       // sx * sy
    long long off3;                        // the first interior cell of a 3-D parent
    double kappa, value, dt;               // T values held in doubles: the constant diffusivity, the mask value, the time step
};

template <typename T, int W, bool GEN, bool FIELD, bool ONCHIP, int NF>
__global__ __launch_bounds__(ONCHIP ? ON_CHIP_LANES : 256) void k_vertical_implicit_diffusion(VdiffPtrs p, VdiffArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    typedef typename Vec<T, W>::aligned_t lvec_t;
    constexpr int LA = LOOKAHEAD<NF>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int j = item / a.cpr;                                    // interior row (0-based)
    const int e0 = (item - j * a.cpr) * W;                         // first interior column of the chunk (0-based)
    const long long row = a.off3 + (long long)a.sx * j + e0;
    const int Nz = a.Nz, n = a.n;
    auto chunk = [](const T* q) { return *reinterpret_cast<const cvec_t*>(q); };

    T* x[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        x[f] = static_cast<T*>(p.x[f]) + row;                      // entries f >= n are never dereferenced
        // sixteen fields: the item's pointers are held as lane values, to which a level adds ONE wave-uniform offset; left alone the compiler
        // keeps sixteen uniform (base + level offset) pairs per level in flight and runs out of scalar registers
        if constexpr (NF > 4) asm volatile("" : "+v"(x[f]));
    }
    const T* dzc = static_cast<const T*>(p.dzc);
    const T* dzf = static_cast<const T*>(p.dzf);
    const T* ktab = static_cast<const T*>(p.kappa);                                   // PROFILE
    const T* kfld = FIELD ? static_cast<const T*>(p.kappa) + row : nullptr;           // FIELD: face k (0-based: under cell k) at plane Hz + k
    const T dt = (T)a.dt, one = T(1), mval = (T)a.value, kconst = (T)a.kappa;
    const T small = T(10) * std::numeric_limits<T>::epsilon();

    // t[k], k = 1 .. Nz - 1 (0-based): the storage policy
    lvec_t* tl = reinterpret_cast<lvec_t*>(lds_raw) + threadIdx.x;                    // [level][lane]
    T* tg = ONCHIP ? nullptr : static_cast<T*>(p.t) + row;
    auto put_t = [&](int k, cvec_t v) {
        if constexpr (ONCHIP) tl[k * ON_CHIP_LANES] = v;
        else *reinterpret_cast<cvec_t*>(tg + a.plane * k) = v;
    };
    auto get_t = [&](int k) -> cvec_t {
        if constexpr (ONCHIP) return tl[k * ON_CHIP_LANES];
        else return chunk(tg + a.plane * k);
    };

    int m[W];                                                      // masked levels (0-based k < m): the first wet cell is m
#pragma unroll
    for (int e = 0; e < W; ++e) m[e] = 0;
    if (p.counts) {
        const Counts<W> c = *reinterpret_cast<const Counts<W>*>(p.counts + (long long)a.Nx * j + e0);
#pragma unroll
        for (int e = 0; e < W; ++e) m[e] = min(max(c[e], 0), Nz);
    }

    // ---- upwards: the elimination ------------------------------------------------------------------------------------------------------------
    struct Level {
        cvec_t f[NF];                                              // the right-hand sides at level k
        cvec_t kap;                                                // FIELD: kappa at the level's top face
        T kp, dc, df;                                              // otherwise kappa there; dz_c[k]; dz_f of the top face
    };
    auto load = [&](Level& L, int k) {
        const int kt = min(k + 1, Nz - 1);                         // the top face (0-based: over cell k); the closed one clamped onto the last open one
        L.dc = dzc[k];
        L.df = dzf[kt];
        L.kp = kconst;
        if (Nz > 1) {                                              // one level: no open face, nothing of kappa is loaded
            if constexpr (FIELD) L.kap = chunk(kfld + a.plane * kt);
            else if (a.profile) L.kp = ktab[kt];
        }
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (f < n) L.f[f] = chunk(x[f] + a.plane * k);
    };

    T phi[NF][W];                                                  // carried: phi of the level below, per field
    T beta[W], upb[W], kb[W];                                      // carried: beta, up of the level below; kappa at the bottom face
    T dfb = one;                                                   // carried: dz_f of the bottom face
#pragma unroll
    for (int e = 0; e < W; ++e) {
        beta[e] = one; upb[e] = T(0); kb[e] = T(0);
#pragma unroll
        for (int f = 0; f < NF; ++f) phi[f][e] = T(0);
    }

    Level ring[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) load(ring[s], min(s, Nz - 1));
    for (int k0 = 0; k0 < Nz; k0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int k = k0 + s;
            if (k >= Nz) break;
            Level L = ring[s];
            if (k + LA < Nz) load(ring[s], k + LA);                // level k + LA goes out before level k's arithmetic
            const bool open_up = k + 1 < Nz;
            cvec_t tv;
            T lo[W];
            bool open_lo[W];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                T kt = L.kp;
                if constexpr (FIELD) kt = L.kap[e];
                // the coefficients of a closed face are formed on carried or clamped values and never used
                const T up = -(dt * ((kt / L.dc) / L.df));
                lo[e] = -(dt * ((kb[e] / L.dc) / dfb));
                open_lo[e] = k > m[e];
                const T diag = open_up ? (open_lo[e] ? (one - up) - lo[e] : one - up) : (open_lo[e] ? one - lo[e] : one);
                const T t = open_lo[e] ? upb[e] / beta[e] : T(0);
                beta[e] = open_lo[e] ? diag - lo[e] * t : diag;
                tv[e] = t;
                upb[e] = up;
                kb[e] = kt;
            }
            dfb = L.df;
            if (k > 0) put_t(k, tv);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                if (f >= n) continue;
                cvec_t out;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const T fv = L.f[f][e];
                    // one division serves both rows: f / beta in the bottom row of the wet column, (f - lo phi) / beta above it
                    const T num = open_lo[e] ? fv - lo[e] * phi[f][e] : fv;
                    const bool elide = open_lo[e] && !(__builtin_elementwise_abs(beta[e]) > small);
                    const T r = k < m[e] ? mval : (elide ? fv : num / beta[e]);
                    phi[f][e] = r;
                    out[e] = r;
                }
                *reinterpret_cast<cvec_t*>(x[f] + a.plane * k) = out;                  // re-read on the way down: an ordinary store
            }
        }
    }

    // ---- downwards: the back substitution, levels Nz - 2 .. the chunk's lowest wet level; phi holds level Nz - 1 -----------------------------------
    int mmin = m[0];
#pragma unroll
    for (int e = 1; e < W; ++e) mmin = min(mmin, m[e]);
    const int nb = Nz - 1 - mmin;                                  // levels to substitute: q = 0 .. nb - 1 is level Nz - 2 - q
    if (nb <= 0) return;
    struct Back {
        cvec_t f[NF];                                              // the forward phi at level k
        cvec_t t;                                                  // t[k + 1]
    };
    auto loadb = [&](Back& B, int k) {
        B.t = get_t(k + 1);
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (f < n) B.f[f] = chunk(x[f] + a.plane * k);
    };
    Back rb[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) loadb(rb[s], max(Nz - 2 - s, mmin));
    for (int q0 = 0; q0 < nb; q0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int q = q0 + s;
            if (q >= nb) break;
            const int k = Nz - 2 - q;
            Back B = rb[s];
            if (q + LA < nb) loadb(rb[s], k - LA);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                if (f >= n) continue;
                cvec_t out;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const T v = B.f[f][e];
                    const T r = k >= m[e] ? v - B.t[e] * phi[f][e] : v;               // under the bottom: the mask value, as it stands
                    phi[f][e] = r;
                    out[e] = r;
                }
                store_chunk<NT>(reinterpret_cast<cvec_t*>(x[f] + a.plane * k), out);
            }
        }
    }
}

bool known_ft(int ft) { return ft == TPG_F32 || ft == TPG_F64; }

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_vertical_diffusion_last_error(void) { return tpg_last_error(); }

int tpg_vertical_diffusion_on_chip_levels(int n, int ft)
{
    if (!known_ft(ft)) { tpg::set_error("unknown element type ft=%d", ft); return TPG_ERR_INVALID_ARGUMENT; }
    if (n < 1 || n > TPG_MAX_FIELDS) { tpg::set_error("%d fields: 1 to TPG_MAX_FIELDS = %d in one call", n, TPG_MAX_FIELDS); return TPG_ERR_INVALID_ARGUMENT; }
    return ON_CHIP_LEVELS;                 // t alone sits in LDS, 16 B per lane and level in either type: the bound does not depend on n
}

int tpg_vertical_implicit_diffusion(void* const fields[], int n, const void* kappa, double kappa_value, int kappa_form, const void* dz_c,
                                    const void* dz_f, const int32_t* counts, double mask_value, double dt, void* scratch, int path, int Nx,
                                    int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (!fields || n < 1) { tpg::set_error("no fields"); return TPG_ERR_INVALID_ARGUMENT; }
    if (n > TPG_MAX_FIELDS) { tpg::set_error("%d fields: at most TPG_MAX_FIELDS = %d in one call", n, TPG_MAX_FIELDS); return TPG_ERR_INVALID_ARGUMENT; }
    for (int f = 0; f < n; ++f)
        if (!fields[f]) { tpg::set_error("null field %d", f); return TPG_ERR_INVALID_ARGUMENT; }
    if (kappa_form != TPG_KAPPA_CONSTANT && kappa_form != TPG_KAPPA_PROFILE && kappa_form != TPG_KAPPA_FIELD) {
        tpg::set_error("kappa form %d is not built (TPG_KAPPA_CONSTANT = 0, TPG_KAPPA_PROFILE = 1 and TPG_KAPPA_FIELD = 2 are)", kappa_form);
        return TPG_ERR_UNSUPPORTED;
    }
    if (path != TPG_VDIFF_AUTO && path != TPG_VDIFF_ON_CHIP && path != TPG_VDIFF_STREAMED) {
        tpg::set_error("path %d is not built (TPG_VDIFF_AUTO = 0, TPG_VDIFF_ON_CHIP = 1 and TPG_VDIFF_STREAMED = 2 are)", path);
        return TPG_ERR_UNSUPPORTED;
    }
    const bool constant = kappa_form == TPG_KAPPA_CONSTANT, field = kappa_form == TPG_KAPPA_FIELD;
    if (constant && kappa) { tpg::set_error("kappa given with TPG_KAPPA_CONSTANT: the diffusivity is kappa_value"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!constant && !kappa) { tpg::set_error("null kappa with %s", field ? "TPG_KAPPA_FIELD" : "TPG_KAPPA_PROFILE"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!dz_c || !dz_f) { tpg::set_error("null dz_c or dz_f"); return TPG_ERR_INVALID_ARGUMENT; }
    if (path == TPG_VDIFF_STREAMED && !scratch) { tpg::set_error("TPG_VDIFF_STREAMED without scratch"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!std::isfinite(dt)) { tpg::set_error("dt is not finite"); return TPG_ERR_INVALID_ARGUMENT; }
    if (constant && !std::isfinite(kappa_value)) { tpg::set_error("kappa_value is not finite"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    for (int f = 0; f < n; ++f)
        if (misaligned(esz, fields[f])) { tpg::set_error("field %d: pointer not aligned to its element type", f); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(esz, kappa, dz_c, dz_f, scratch)) { tpg::set_error("kappa, dz_c, dz_f or scratch pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(4, counts)) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz;
    Span spans[TPG_MAX_FIELDS + 2];
    for (int f = 0; f < n; ++f) {
        spans[f] = Span{ fields[f], bytes, "", true };
        snprintf(spans[f].name, sizeof spans[f].name, "field %d", f);
    }
    spans[n] = Span{ scratch, bytes, "scratch", true };
    spans[n + 1] = Span{ kappa, field ? bytes : (unsigned long long)(Nz + 1) * esz, "kappa", false };
    // a field against the other fields, scratch and a FIELD kappa; scratch against kappa in either form
    if (int rc = check_overlaps(spans, n + (field ? 2 : 1), "an item writes its own cells while other items read theirs")) return rc;
    if (!field)
        if (int rc = check_overlaps(spans + n, 2, "an item writes its own cells while other items read theirs")) return rc;
    // AUTO: with scratch the streamed path, which the measurements favour (at 75 levels the on-chip path holds two waves per CU and takes 1.8
    // to 2.0 times as long for one field); without scratch the on-chip path, or the refusal below
    const bool on_chip = path == TPG_VDIFF_ON_CHIP || (path == TPG_VDIFF_AUTO && !scratch);
    if (on_chip && Nz > ON_CHIP_LEVELS) {
        tpg::set_error("Nz = %d is beyond the on-chip path's %d levels (tpg_vertical_diffusion_on_chip_levels): pass scratch and "
                       "TPG_VDIFF_STREAMED or TPG_VDIFF_AUTO", Nz, ON_CHIP_LEVELS);
        return TPG_ERR_UNSUPPORTED;
    }
    if ((long long)Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("vertical implicit diffusion: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }

    VdiffPtrs p{};
    void* all[TPG_MAX_FIELDS + 2];
    int na = 0;
    for (int f = 0; f < n; ++f) { p.x[f] = fields[f]; all[na++] = fields[f]; }
    p.kappa = kappa; p.dzc = dz_c; p.dzf = dz_f; p.counts = counts; p.t = on_chip ? nullptr : scratch;
    if (!on_chip) all[na++] = scratch;
    if (field) all[na++] = const_cast<void*>(kappa);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, all, na);
        const int cpr = Nx / cp.W;
        const VdiffArgs a{ Nx, Ny, Nz, g.sx, cpr, Ny * cpr, n, kappa_form == TPG_KAPPA_PROFILE, g.plane, interior3(g),
                           constant ? (double)(T)kappa_value : 0.0, counts ? (double)(T)mask_value : 0.0, (double)(T)dt };
        int status = TPG_OK;
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto go = [&](auto fld, auto chip, auto nf) {
                constexpr bool ONCHIP = decltype(chip)::value;
                auto kernel = k_vertical_implicit_diffusion<T, W, GEN, decltype(fld)::value, ONCHIP, decltype(nf)::value>;
                const int lanes = ONCHIP ? ON_CHIP_LANES : 256;
                const size_t lds = ONCHIP ? (size_t)Nz * ON_CHIP_LANES * W * sizeof(T) : 0;
                if (lds > 64 * 1024) {                             // more dynamic LDS than a launch gets by default: ask for it (a host-side attribute, no stream work)
                    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES)) {
                        tpg::set_error("k_vertical_implicit_diffusion: %s asking for %d B of LDS (hipError_t %d)", hipGetErrorString(e), LDS_BYTES, (int)e);
                        status = (int)e;
                        return;
                    }
                }
                hipLaunchKernelGGL(kernel, dim3((unsigned)((a.items + lanes - 1) / lanes)), dim3(lanes), lds, st, p, a);
            };
            auto by_n = [&](auto fld, auto chip) {
                if (n == 1)      go(fld, chip, std::integral_constant<int, 1>{});
                else if (n == 2) go(fld, chip, std::integral_constant<int, 2>{});
                else if (n <= 4) go(fld, chip, std::integral_constant<int, 4>{});
                else             go(fld, chip, std::integral_constant<int, TPG_MAX_FIELDS>{});
            };
            if (field) { if (on_chip) by_n(std::true_type{}, std::true_type{}); else by_n(std::true_type{}, std::false_type{}); }
            else       { if (on_chip) by_n(std::false_type{}, std::true_type{}); else by_n(std::false_type{}, std::false_type{}); }
        });
        if (status != TPG_OK) return status;
        return tpg::launch_status("k_vertical_implicit_diffusion");
    });
}

}  // extern "C"
