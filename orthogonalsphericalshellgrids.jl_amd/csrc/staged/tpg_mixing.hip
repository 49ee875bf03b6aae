// tpg_mixing.hip -- the vertical mixing diffusivities of a hydrostatic model for gfx950: convective adjustment
// (tpg_convective_adjustment_diffusivities) and Richardson-number-based mixing (tpg_ri_based_diffusivities), written at the three
// locations tpg_vertical_implicit_diffusion wants a TPG_KAPPA_FIELD at: kappa and nu at (Center, Center, Face), and nu interpolated to
// the columns of u and of v.  Called after the AB2 update and before the three implicit calls.
// [recalled: Oceananigans' ConvectiveAdjustmentVerticalDiffusivity and RiBasedVerticalDiffusivity with PiecewiseLinearRiDependentTapering;
// parity unpinned, like every operator here]
//
// THE RULE is written out once, in tripolar_hip_mixing.h beside this file.  Evaluated in the field type T with no contraction; every
// operation is one correctly rounded IEEE operation.
//
// Stream-bound, of the family of the hydrostatic and free-surface kernels: a work item is ONE chunk of W interior columns of one row and
// walks the faces 1..Nz+1 upwards.  It carries the cells of level k - 1 in registers, so every plane of b, u and v is fetched once for
// the vertical differences.  For kappa_u it also forms nu_c of the column west of its chunk, for kappa_v of the W columns south of it, by
// the same sequence of operations on cells it loads itself: the neighbour item's bits, with no exchange and no second pass.  What an
// absent output would need is not loaded (a wave-uniform test of the output pointers).
// Compile-time forms: the element type, the chunk form (W, GEN) and the closure (RI: the Ri rule; otherwise convective adjustment, which
// never touches u, v or the *_prev arrays).  The outputs, the time average and the count planes are wave-uniform run-time switches.
// Items are numbered (row, chunk) with the chunk fastest, 256 to a block.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  Nothing shared between items, no LDS, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "tripolar_hip_mixing.h"
#include <cmath>

// compile-time switch of profiles/mixing/ (make -C staged mixing MIXING_TAG=_nt0 MIXING_FLAGS=-DTPG_MIX_NT=0)
#ifndef TPG_MIX_NT
#define TPG_MIX_NT 1
#endif

namespace {

constexpr bool NT = TPG_MIX_NT;            // the outputs go out in streaming stores

struct MixPtrs {
    const void *b, *u, *v;                 // u, v: the Ri rule only
    const void *kprev, *nprev;             // the Ri rule's time average, both or neither
    void *kc, *nc, *ku, *kv;               // the outputs, null each where absent
    const void* dz_f;
    const int32_t *n_cc, *n_fc, *n_cf;     // null, or Ny x Nx planes
};

struct MixArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int items;                             // Ny x cpr
    long long plane;                       // sx * sy
    long long off3;                        // plane * Hz + sx * Hy + Hx: the first interior cell of a parent
    // T values held in doubles.  Convective adjustment: background kappa, convective kappa, background nu, convective nu.
    // The Ri rule: nu0, kappa0, kappa_ca, Ri0, Ri_delta, Cav, one + T(Cav).
    double q[7];
    double value;                          // the mask value
};

// the cells of one level an item works on: the row with the column west of the chunk (index 0 is column e0 - 1), the row south, and of v
// the row north
template <typename T, int W>
struct Cells {
    T b[W + 1], bs[W];                     // row j, columns e0-1 .. e0+W-1; row j-1, columns e0 .. e0+W-1
    T u[W + 2], us[W + 1];                 // row j, columns e0-1 .. e0+W;   row j-1, columns e0 .. e0+W
    T v[W + 1], vn[W + 1], vs[W];          // rows j and j+1, columns e0-1 .. e0+W-1; row j-1, columns e0 .. e0+W-1
};

template <typename T> struct Rule { T q[7]; bool avg; };

// nu_c and kappa of one column at one face from its own cells: THE fixed sequence of operations (tripolar_hip_mixing.h)
template <typename T, bool RI>
__device__ __forceinline__ void diffusivities(const Rule<T>& r, T b_hi, T b_lo, T u0_hi, T u0_lo, T u1_hi, T u1_lo, T v0_hi, T v0_lo, T v1_hi,
                                              T v1_lo, T dz, T nprev, T kprev, T& nu, T& kappa)
{
    const T half = T(0.5), one = T(1);
    const T N2 = (b_hi - b_lo) / dz;
    if constexpr (!RI) {
        const bool stable = N2 >= T(0);
        kappa = stable ? r.q[0] : r.q[1];
        nu = stable ? r.q[2] : r.q[3];
    } else {
        const T du0 = (u0_hi - u0_lo) / dz, du1 = (u1_hi - u1_lo) / dz;
        const T dv0 = (v0_hi - v0_lo) / dz, dv1 = (v1_hi - v1_lo) / dz;
        const T su = du0 * du0 + du1 * du1;
        const T sv = dv0 * dv0 + dv1 * dv1;
        const T S2 = half * su + half * sv;
        const T Ri = N2 == T(0) ? T(0) : N2 / S2;
        const T x = (Ri - r.q[3]) / r.q[4];
        const T y = x > T(0) ? x : T(0);
        const T z = y < one ? y : one;
        const T tau = one - z;
        nu = r.q[0] * tau;
        kappa = r.q[1] * tau;
        if (N2 < T(0)) kappa = kappa + r.q[2];
        if (r.avg) {
            nu = (r.q[5] * nprev + nu) / r.q[6];
            kappa = (r.q[5] * kprev + kappa) / r.q[6];
        }
    }
}

template <typename T, int W, bool GEN, bool RI>
__global__ __launch_bounds__(256) void k_mixing_diffusivities(MixPtrs p, MixArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int j = item / a.cpr;                                    // the interior row (0-based)
    const int e0 = (item - j * a.cpr) * W;                         // first interior column of the chunk (0-based)
    const int Nz = a.Nz, sx = a.sx;
    const bool west = p.ku != nullptr, south = p.kv != nullptr;    // what an absent output would need is not loaded
    const bool want_kappa = p.kc != nullptr, want_nu = p.nc || west || south;
    auto chunk = [](const T* q) { return *reinterpret_cast<const cvec_t*>(q); };

    Rule<T> rule;
#pragma unroll
    for (int n = 0; n < 7; ++n) rule.q[n] = (T)a.q[n];
    rule.avg = RI && p.kprev != nullptr;
    const T mv = (T)a.value, half = T(0.5);

    // masked faces: k <= m + 1 (1-based); -1 without a count plane: no face
    int mc[W], mu[W], mw[W];
#pragma unroll
    for (int e = 0; e < W; ++e) mc[e] = mu[e] = mw[e] = -1;
    const long long n0 = (long long)a.Nx * j + e0;                 // a count plane has no halo
    auto counts = [&](const int32_t* plane, int (&m)[W]) {
        const Counts<W> n = *reinterpret_cast<const Counts<W>*>(plane + n0);
#pragma unroll
        for (int e = 0; e < W; ++e) m[e] = min(max(n[e], 0), Nz);
    };
    if (p.n_cc && (p.kc || p.nc)) counts(p.n_cc, mc);
    if (p.n_fc && p.ku) counts(p.n_fc, mu);
    if (p.n_cf && p.kv) counts(p.n_cf, mw);

    const long long f0 = a.off3 + (long long)sx * j + e0;         // the chunk's first cell at level 1 / face 1
    const T* b = static_cast<const T*>(p.b) + f0;
    const T* u = RI ? static_cast<const T*>(p.u) + f0 : nullptr;
    const T* v = RI ? static_cast<const T*>(p.v) + f0 : nullptr;
    const T* kprev = rule.avg ? static_cast<const T*>(p.kprev) + f0 : nullptr;
    const T* nprev = rule.avg ? static_cast<const T*>(p.nprev) + f0 : nullptr;
    const T* dzf = static_cast<const T*>(p.dz_f);
    auto out_at = [&](void* q) { return q ? static_cast<T*>(q) + f0 : nullptr; };
    T* kc = out_at(p.kc);
    T* nc = out_at(p.nc);
    T* ku = out_at(p.ku);
    T* kv = out_at(p.kv);

    // the cells of level k (1-based): plane k - 1 above the chunk's first
    auto load = [&](Cells<T, W>& L, int k) {
        const long long at = a.plane * (k - 1);
        const cvec_t bc = chunk(b + at);
        cvec_t bs = cvec_t{};
        if (south) bs = chunk(b + at - sx);
        L.b[0] = west ? b[at - 1] : T(0);
#pragma unroll
        for (int e = 0; e < W; ++e) { L.b[e + 1] = bc[e]; L.bs[e] = bs[e]; }
        if constexpr (RI) {
            const cvec_t uc = chunk(u + at), vc = chunk(v + at), vn = chunk(v + at + sx);
            cvec_t us = cvec_t{}, vs = cvec_t{};
            L.u[W + 1] = u[at + W];
            L.u[0] = L.v[0] = L.vn[0] = L.us[W] = T(0);
            if (west) { L.u[0] = u[at - 1]; L.v[0] = v[at - 1]; L.vn[0] = v[at + sx - 1]; }
            if (south) { us = chunk(u + at - sx); vs = chunk(v + at - sx); L.us[W] = u[at - sx + W]; }
#pragma unroll
            for (int e = 0; e < W; ++e) { L.u[e + 1] = uc[e]; L.us[e] = us[e]; L.v[e + 1] = vc[e]; L.vn[e + 1] = vn[e]; L.vs[e] = vs[e]; }
        }
    };
    // one face of the outputs: the values, or the mask value under the column's first open face
    auto store = [&](T* out, int k, const T (&val)[W], const int (&m)[W]) {
        if (!out) return;
        cvec_t o;
#pragma unroll
        for (int e = 0; e < W; ++e) o[e] = k <= m[e] + 1 ? mv : val[e];
        store_chunk<NT>(reinterpret_cast<cvec_t*>(out + a.plane * (k - 1)), o);
    };
    T zero[W];
#pragma unroll
    for (int e = 0; e < W; ++e) zero[e] = T(0);
    auto closed_face = [&](int k) { store(kc, k, zero, mc); store(nc, k, zero, mc); store(ku, k, zero, mu); store(kv, k, zero, mw); };

    closed_face(1);
    Cells<T, W> lo{}, hi{};
    if (Nz > 1) load(lo, 1);
    for (int k = 2; k <= Nz; ++k) {
        load(hi, k);
        const T dz = dzf[k - 1];
        const long long at = a.plane * (k - 1);
        cvec_t pk = cvec_t{}, pn = cvec_t{}, pns = cvec_t{};
        T pnw = T(0);
        if (rule.avg) {
            if (want_kappa) pk = chunk(kprev + at);
            if (want_nu) pn = chunk(nprev + at);
            if (west) pnw = nprev[at - 1];
            if (south) pns = chunk(nprev + at - sx);
        }
        T nu[W + 1], kappa[W], nus[W], unused;                     // nu: index 0 is the column west of the chunk
#pragma unroll
        for (int e = 0; e < W; ++e) {
            diffusivities<T, RI>(rule, hi.b[e + 1], lo.b[e + 1], hi.u[e + 1], lo.u[e + 1], hi.u[e + 2], lo.u[e + 2], hi.v[e + 1], lo.v[e + 1],
                                 hi.vn[e + 1], lo.vn[e + 1], dz, pn[e], pk[e], nu[e + 1], kappa[e]);
            nus[e] = T(0);
            if (south)                                             // the column south: its v faces are v[j-1] and this row's v[j]
                diffusivities<T, RI>(rule, hi.bs[e], lo.bs[e], hi.us[e], lo.us[e], hi.us[e + 1], lo.us[e + 1], hi.vs[e], lo.vs[e], hi.v[e + 1],
                                     lo.v[e + 1], dz, pns[e], T(0), nus[e], unused);
        }
        nu[0] = T(0);
        if (west)
            diffusivities<T, RI>(rule, hi.b[0], lo.b[0], hi.u[0], lo.u[0], hi.u[1], lo.u[1], hi.v[0], lo.v[0], hi.vn[0], lo.vn[0], dz, pnw, T(0),
                                 nu[0], unused);
        T nuc[W], nuu[W], nuv[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            nuc[e] = nu[e + 1];
            nuu[e] = half * (nu[e] + nu[e + 1]);
            nuv[e] = half * (nus[e] + nu[e + 1]);
        }
        store(kc, k, kappa, mc);
        store(nc, k, nuc, mc);
        store(ku, k, nuu, mu);
        store(kv, k, nuv, mw);
        lo = hi;
    }
    closed_face(Nz + 1);
}

// the checks both entry points share, in the header's order, and the launch
struct MixCall {
    const char* name;
    bool ri;
    const void *b, *u, *v, *kprev, *nprev;
    void *kc, *nc, *ku, *kv;
    const char* const* pnames;             // the names of the parameters, in the order of the argument list
    const double* params;
    int nparams;
    const void* dz_f;
    const int32_t *n_cc, *n_fc, *n_cf;
    double mask_value;
};

int mixing_call(const MixCall& c, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    const int INVALID = TPG_ERR_INVALID_ARGUMENT, UNSUPPORTED = TPG_ERR_UNSUPPORTED;
    // 1. the geometry
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    // 2. the null combinations
    if (!c.b) { tpg::set_error("null b"); return INVALID; }
    if (c.ri && (!c.u || !c.v)) { tpg::set_error("null u or v"); return INVALID; }
    if (!c.dz_f) { tpg::set_error("null dz_f"); return INVALID; }
    if (!c.kc && !c.nc && !c.ku && !c.kv) { tpg::set_error("no output: kappa_c, nu_c, kappa_u and kappa_v are all null"); return INVALID; }
    if (c.ri && !c.kprev != !c.nprev) {
        tpg::set_error("%s without %s: the time average takes both or neither", c.kprev ? "kappa_c_prev" : "nu_c_prev", c.kprev ? "nu_c_prev" : "kappa_c_prev");
        return INVALID;
    }
    // 3. the numbers
    const bool f64 = ft == TPG_F64;
    auto finite = [&](double x) { return f64 ? std::isfinite(x) : std::isfinite((float)x); };       // as the element type holds it
    for (int n = 0; n < c.nparams; ++n)
        if (!finite(c.params[n])) { tpg::set_error("%s is not finite", c.pnames[n]); return INVALID; }
    if ((c.n_cc || c.n_fc || c.n_cf) && !finite(c.mask_value)) { tpg::set_error("mask_value is not finite"); return INVALID; }
    double den = 0.0;
    if (c.ri) {
        const double delta = f64 ? c.params[4] : (double)(float)c.params[4];
        if (!(delta > 0)) { tpg::set_error("Ri_delta = %g is not positive (as the element type holds it)", c.params[4]); return INVALID; }
        den = f64 ? 1.0 + c.params[5] : (double)(1.0f + (float)c.params[5]);                 // one + T(Cav), formed once, in T
        if (c.kprev && den == 0) { tpg::set_error("1 + Cav == 0: the time average divides by it"); return INVALID; }
    }
    // 4. alignment
    const size_t esz = elem_size(ft);
    if (misaligned(esz, c.b, c.u, c.v, c.kprev, c.nprev)) { tpg::set_error("b, u, v, kappa_c_prev or nu_c_prev pointer not aligned to its element type"); return INVALID; }
    if (misaligned(esz, c.kc, c.nc, c.ku, c.kv)) { tpg::set_error("kappa_c, nu_c, kappa_u or kappa_v pointer not aligned to its element type"); return INVALID; }
    if (misaligned(esz, c.dz_f)) { tpg::set_error("dz_f pointer not aligned to its element type"); return INVALID; }
    if (misaligned(4, c.n_cc, c.n_fc, c.n_cf)) { tpg::set_error("count plane pointer not aligned to int32"); return INVALID; }
    // 5. the overlaps: every output against every other array of the call
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long cells = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz, faces = (unsigned long long)g.plane * (Nz + 1 + 2 * Hz) * esz;
    const unsigned long long cbytes = (unsigned long long)Nx * Ny * 4;
    const Span spans[] = { { c.b, cells, "b", false }, { c.u, cells, "u", false }, { c.v, cells, "v", false },
                           { c.kprev, faces, "kappa_c_prev", false }, { c.nprev, faces, "nu_c_prev", false },
                           { c.kc, faces, "kappa_c", true }, { c.nc, faces, "nu_c", true }, { c.ku, faces, "kappa_u", true }, { c.kv, faces, "kappa_v", true },
                           { c.dz_f, (unsigned long long)(Nz + 1) * esz, "dz_f", false }, { c.n_cc, cbytes, "n_cc", false },
                           { c.n_fc, cbytes, "n_fc", false }, { c.n_cf, cbytes, "n_cf", false } };
    if (int rc = check_overlaps(spans, (int)(sizeof(spans) / sizeof(spans[0])), "every item reads its neighbours' cells while they write: the caller ping-pongs"))
        return rc;
    // 6. the stencil
    if (Hx < 1 || Hy < 1) {
        tpg::set_error("the rule reads b, u, v and the *_prev arrays one cell west, east, south and north of the interior: Hx >= 1 and Hy >= 1 "
                       "needed (halo (%d,%d,%d))", Hx, Hy, Hz);
        return UNSUPPORTED;
    }
    // 7. the work items
    // (the plane check of 1. refuses every such geometry first: Nx * Ny < 2^31 there; kept for a change of either bound)
    if ((long long)Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("%s: too many work items for 32-bit indexing", c.name); return UNSUPPORTED; }

    MixPtrs p{ c.b, c.u, c.v, c.kprev, c.nprev, c.kc, c.nc, c.ku, c.kv, c.dz_f, c.n_cc, c.n_fc, c.n_cf };
    void* arrays[9];
    int na = 0;
    for (const void* x : { c.b, c.u, c.v, c.kprev, c.nprev, (const void*)c.kc, (const void*)c.nc, (const void*)c.ku, (const void*)c.kv })
        if (x) arrays[na++] = const_cast<void*>(x);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        MixArgs a{ Nx, Ny, Nz, g.sx, cpr, Ny * cpr, g.plane, interior3(g), {}, (double)(T)c.mask_value };
        for (int n = 0; n < c.nparams; ++n) a.q[n] = (double)(T)c.params[n];
        a.q[6] = den;
        const unsigned blocks = (unsigned)((a.items + 255) / 256);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            if (c.ri) hipLaunchKernelGGL((k_mixing_diffusivities<T, W, GEN, true>), dim3(blocks), dim3(256), 0, st, p, a);
            else      hipLaunchKernelGGL((k_mixing_diffusivities<T, W, GEN, false>), dim3(blocks), dim3(256), 0, st, p, a);
        });
        return tpg::launch_status("k_mixing_diffusivities");
    });
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_mixing_last_error(void) { return tpg_last_error(); }

int tpg_convective_adjustment_diffusivities(const void* b, void* kappa_c, void* nu_c, void* kappa_u, void* kappa_v, double background_kappa,
                                            double convective_kappa, double background_nu, double convective_nu, const void* dz_f,
                                            const int32_t* n_cc, const int32_t* n_fc, const int32_t* n_cf, double mask_value, int Nx, int Ny,
                                            int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    static const char* const names[] = { "background_kappa", "convective_kappa", "background_nu", "convective_nu" };
    const double params[] = { background_kappa, convective_kappa, background_nu, convective_nu };
    const MixCall c{ "convective adjustment diffusivities", false, b, nullptr, nullptr, nullptr, nullptr, kappa_c, nu_c, kappa_u, kappa_v,
                     names, params, 4, dz_f, n_cc, n_fc, n_cf, mask_value };
    return mixing_call(c, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream);
}

int tpg_ri_based_diffusivities(const void* b, const void* u, const void* v, const void* kappa_c_prev, const void* nu_c_prev, void* kappa_c,
                               void* nu_c, void* kappa_u, void* kappa_v, double nu0, double kappa0, double kappa_ca, double Ri0,
                               double Ri_delta, double Cav, const void* dz_f, const int32_t* n_cc, const int32_t* n_fc, const int32_t* n_cf,
                               double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    static const char* const names[] = { "nu0", "kappa0", "kappa_ca", "Ri0", "Ri_delta", "Cav" };
    const double params[] = { nu0, kappa0, kappa_ca, Ri0, Ri_delta, Cav };
    const MixCall c{ "Ri-based diffusivities", true, b, u, v, kappa_c_prev, nu_c_prev, kappa_c, nu_c, kappa_u, kappa_v, names, params, 6, dz_f,
                     n_cc, n_fc, n_cf, mask_value };
    return mixing_call(c, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream);
}

}  // extern "C"
