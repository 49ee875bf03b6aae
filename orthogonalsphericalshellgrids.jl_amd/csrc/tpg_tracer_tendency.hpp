// tpg_tracer_tendency.hpp -- what the flux-form tracer tendencies share (tpg_advection.hip: centred; tpg_weno.hip: WENO5 in x and y;
// tpg_weno_xyz.hip: WENO5 in x, y and z; each is a library of its own): the pointer struct every tracer kernel takes (TracerPtrs), and on
// the host side the argument record of a call with its checks, the array list for chunk_plan, the pointer struct's fill and the greedy
// split of the tracers into groups.  No device code: a kernel and its Args stay in its file (the WENO5 kernel, its Args and the launch of
// its two calls in tpg_weno_tracer_kernel.hpp, which two of the files include), and so do tpg::check_geom, a scheme refusal and the
// centred call's work-item bound.  A further scheme of the tracer tendency starts here.
#pragma once
#include "tpg_operator.hpp"

namespace {

// what every tracer kernel is launched with
struct TracerPtrs {
    const void* c[TPG_MAX_FIELDS];
    void* G[TPG_MAX_FIELDS];
    const void *u, *v, *w;
    const void *dy, *dx, *az, *dz;
    const int32_t* ncc;
};

// the arguments of tpg_tracer_advection_tendency, tpg_weno_tracer_advection_tendency and tpg_weno_xyz_tracer_advection_tendency, after
// tpg::check_geom
struct TracerCall {
    const void* const* c;
    void* const* G;
    int nfields;
    const void *u, *v, *w;
    const void *dy_fc, *dx_cf, *az_cc, *dz_c;
    const int32_t* n_cc;
    Geom g;
    int ft;

    // the checks the three calls make, in this order; the rule reads `stencil` of c: Hx, Hy >= hxy and Hz >= hz
    int check(int hxy, int hz, const char* stencil) const
    {
        if (nfields < 1) { tpg::set_error("no tracers (nfields = %d)", nfields); return TPG_ERR_INVALID_ARGUMENT; }
        if (nfields > TPG_MAX_FIELDS) { tpg::set_error("%d tracers: at most TPG_MAX_FIELDS = %d in one call", nfields, TPG_MAX_FIELDS); return TPG_ERR_INVALID_ARGUMENT; }
        if (!c || !G) { tpg::set_error("null table of tracers or of tendencies"); return TPG_ERR_INVALID_ARGUMENT; }
        for (int q = 0; q < nfields; ++q) {
            if (!c[q]) { tpg::set_error("null tracer %d", q); return TPG_ERR_INVALID_ARGUMENT; }
            if (!G[q]) { tpg::set_error("null G of tracer %d", q); return TPG_ERR_INVALID_ARGUMENT; }
        }
        if (!u || !v || !w) { tpg::set_error("null u, v or w"); return TPG_ERR_INVALID_ARGUMENT; }
        if (!dy_fc || !dx_cf || !az_cc || !dz_c) { tpg::set_error("null dy_fc, dx_cf, az_cc or dz_c"); return TPG_ERR_INVALID_ARGUMENT; }
        const size_t esz = elem_size(ft);
        const unsigned long long bytes = (unsigned long long)g.plane * (g.Nz + 2 * g.Hz) * esz;            // c, G, u, v
        const unsigned long long wbytes = (unsigned long long)g.plane * (g.Nz + 1 + 2 * g.Hz) * esz;       // w: one more level
        Span in[TPG_MAX_FIELDS + 3], out[TPG_MAX_FIELDS];
        for (int q = 0; q < nfields; ++q) {
            in[q] = Span{ c[q], bytes, "" };
            out[q] = Span{ G[q], bytes, "", true };
            snprintf(in[q].name, sizeof in[q].name, "tracer %d", q);
            snprintf(out[q].name, sizeof out[q].name, "G of tracer %d", q);
        }
        in[nfields] = Span{ u, bytes, "u" };
        in[nfields + 1] = Span{ v, bytes, "v" };
        in[nfields + 2] = Span{ w, wbytes, "w" };
        for (int q = 0; q < nfields; ++q)
            if (misaligned(esz, in[q].p)) { tpg::set_error("%s: pointer not aligned to its element type", in[q].name); return TPG_ERR_INVALID_ARGUMENT; }
        for (int q = 0; q < nfields; ++q)
            if (misaligned(esz, out[q].p)) { tpg::set_error("%s: pointer not aligned to its element type", out[q].name); return TPG_ERR_INVALID_ARGUMENT; }
        if (misaligned(esz, u, v, w)) { tpg::set_error("u, v or w pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
        if (misaligned(esz, dy_fc, dx_cf, az_cc, dz_c)) {
            tpg::set_error("dy_fc, dx_cf, az_cc or dz_c pointer not aligned to its element type");
            return TPG_ERR_INVALID_ARGUMENT;
        }
        if ((uintptr_t)n_cc % 4) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
        // not check_overlaps: the reason goes on out-against-in only
        for (int q = 0; q < nfields; ++q) {
            for (int s = 0; s < nfields + 3; ++s)
                if (arrays_overlap(out[q].p, out[q].bytes, in[s].p, in[s].bytes)) {
                    tpg::set_error("%s overlaps %s (every item reads cells while its neighbours write)", out[q].name, in[s].name);
                    return TPG_ERR_INVALID_ARGUMENT;
                }
            for (int s = 0; s < q; ++s)
                if (arrays_overlap(out[q].p, out[q].bytes, out[s].p, out[s].bytes)) {
                    tpg::set_error("%s overlaps %s", out[q].name, out[s].name);
                    return TPG_ERR_INVALID_ARGUMENT;
                }
        }
        if (g.Hx < hxy || g.Hy < hxy || g.Hz < hz) {
            tpg::set_error("the rule reads %s, u[i+1, j] and v[i, j+1]: Hx >= %d, Hy >= %d and Hz >= %d needed (halo (%d,%d,%d))", stencil, hxy, hxy, hz,
                           g.Hx, g.Hy, g.Hz);
            return TPG_ERR_UNSUPPORTED;
        }
        return TPG_OK;
    }

    // every array whose chunks the kernels touch, for chunk_plan; returns how many
    int arrays(void* a[2 * TPG_MAX_FIELDS + 6]) const
    {
        int na = 0;
        for (int q = 0; q < nfields; ++q) {
            a[na++] = const_cast<void*>(c[q]);
            a[na++] = G[q];
        }
        for (const void* x : { u, v, w, dy_fc, dx_cf, az_cc }) a[na++] = const_cast<void*>(x);
        return na;
    }

    TracerPtrs pointers() const
    {
        TracerPtrs p{};
        for (int q = 0; q < nfields; ++q) { p.c[q] = c[q]; p.G[q] = G[q]; }
        p.u = u; p.v = v; p.w = w; p.dy = dy_fc; p.dx = dx_cf; p.az = az_cc; p.dz = dz_c; p.ncc = n_cc;
        return p;
    }
};

// the tracers split greedily into whole groups of 4, then of 2, then single ones, up to GROUP (a file's compile-time switch): one
// f(integral_constant<int, TG>, first tracer, number of groups) per group size that occurs, so a lone tracer pays nothing for a group's registers
template <int GROUP, typename F>
void tracer_groups(int nfields, F&& f)
{
    int q0 = 0;
    auto groups_of = [&](auto tg) {                                // the whole groups of TG among the tracers not yet taken
        constexpr int TG = decltype(tg)::value;
        const int n = (nfields - q0) / TG;
        if (n) f(tg, q0, n);
        q0 += n * TG;
    };
    if constexpr (GROUP >= 4) groups_of(std::integral_constant<int, 4>{});
    if constexpr (GROUP >= 2) groups_of(std::integral_constant<int, 2>{});
    groups_of(std::integral_constant<int, 1>{});
}

}  // namespace
