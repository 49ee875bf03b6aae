// tpg_momentum_tendency.hpp -- what the vector-invariant momentum tendencies share (tpg_momentum.hip: enstrophy-conserving;
// tpg_weno_momentum.hip: WENO5-upwinded vorticity term; tpg_weno_vi.hip: upwinded vertical and kinetic-energy terms too; each is a library of
// its own): the pointer struct and the Args every momentum kernel takes (MomentumPtrs, MomentumArgs), and on the host side the argument
// record of a call with its checks, the array list for chunk_plan, the pointer struct's fill, the work-item bound, the Args fill and the
// dispatch.  No device code: a kernel stays in its file (the WENO5 vorticity kernel in tpg_weno_vorticity_kernel.hpp, which two of the
// files include), and so do tpg::check_geom and a scheme refusal.  A further scheme of the momentum tendency starts here.
#pragma once
#include "tpg_operator.hpp"

namespace {

// what every momentum kernel is launched with
struct MomentumPtrs {
    const void *u, *v, *w;
    void *Gu, *Gv;
    const void *dxfc, *dyfc, *azfc, *dxcf, *dycf, *azcf, *azcc, *azff, *dz;
    const int32_t *nfc, *ncf;
};

struct MomentumArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int items;                             // row tiles x cpr
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double value;                          // the mask value (a T value held in a double)
};

// the arguments of tpg_momentum_advection_tendency, tpg_weno_momentum_advection_tendency and tpg_weno_vi_momentum_advection_tendency, after
// tpg::check_geom.  `dz_f` is the call's table of vertical spacings and `dz` what its messages call it (the third call passes dz_c there)
struct MomentumCall {
    const void *u, *v, *w;
    void *Gu, *Gv;
    const void *dx_fc, *dy_fc, *az_fc, *dx_cf, *dy_cf, *az_cf, *az_cc, *az_ff, *dz_f;
    const int32_t *n_fc, *n_cf;
    double mask_value;
    Geom g;
    int ft;
    const char* dz = "dz_f";

    // the checks both calls make, in this order; the rule reads `stencil`: Hx, Hy >= hxy and Hz >= 1
    int check(int hxy, const char* stencil) const
    {
        if (!u || !v || !w) { tpg::set_error("null u, v or w"); return TPG_ERR_INVALID_ARGUMENT; }
        if (!Gu || !Gv) { tpg::set_error("null Gu or Gv"); return TPG_ERR_INVALID_ARGUMENT; }
        if (!dx_fc || !dy_fc || !az_fc || !dx_cf || !dy_cf || !az_cf || !az_cc || !az_ff || !dz_f) {
            tpg::set_error("null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or %s", dz);
            return TPG_ERR_INVALID_ARGUMENT;
        }
        if (!n_fc != !n_cf) { tpg::set_error("the count planes n_fc and n_cf are given together or not at all (%s is null)", n_fc ? "n_cf" : "n_fc"); return TPG_ERR_INVALID_ARGUMENT; }
        const size_t esz = elem_size(ft);
        if (misaligned(esz, u, v, w)) { tpg::set_error("u, v or w pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
        if (misaligned(esz, Gu, Gv)) { tpg::set_error("Gu or Gv pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
        if (misaligned(esz, dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_f)) {
            tpg::set_error("dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or %s pointer not aligned to its element type", dz);
            return TPG_ERR_INVALID_ARGUMENT;
        }
        if ((uintptr_t)n_fc % 4 || (uintptr_t)n_cf % 4) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
        const unsigned long long bytes = (unsigned long long)g.plane * (g.Nz + 2 * g.Hz) * esz;            // u, v, Gu, Gv
        const unsigned long long wbytes = (unsigned long long)g.plane * (g.Nz + 1 + 2 * g.Hz) * esz;       // w: one more level
        const Span in[3] = { { u, bytes, "u" }, { v, bytes, "v" }, { w, wbytes, "w" } };
        const Span out[2] = { { Gu, bytes, "Gu" }, { Gv, bytes, "Gv" } };
        // not check_overlaps: the reason goes on out-against-in only
        for (const Span& o : out)
            for (const Span& s : in)
                if (arrays_overlap(o.p, o.bytes, s.p, s.bytes)) {
                    tpg::set_error("%s overlaps %s (every item reads cells while its neighbours write)", o.name, s.name);
                    return TPG_ERR_INVALID_ARGUMENT;
                }
        if (arrays_overlap(Gv, bytes, Gu, bytes)) { tpg::set_error("Gv overlaps Gu"); return TPG_ERR_INVALID_ARGUMENT; }
        if (g.Hx < hxy || g.Hy < hxy || g.Hz < 1) {
            tpg::set_error("the rule reads %s: Hx >= %d, Hy >= %d and Hz >= 1 needed (halo (%d,%d,%d))", stencil, hxy, hxy, g.Hx, g.Hy, g.Hz);
            return TPG_ERR_UNSUPPORTED;
        }
        return TPG_OK;
    }

    // every array whose chunks the kernels touch, for chunk_plan; returns how many
    int arrays(void* a[13]) const
    {
        int na = 0;
        for (const void* x : { u, v, w, (const void*)Gu, (const void*)Gv, dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff }) a[na++] = const_cast<void*>(x);
        return na;
    }

    MomentumPtrs pointers() const { return MomentumPtrs{ u, v, w, Gu, Gv, dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_f, n_fc, n_cf }; }

    // ONE launch of a file's kernel over (row tile, chunk) items, 256 to a block, with its rows per item in Float64 and Float32.
    // kernel_of(T(), integral_constant<int, W>, bool_constant<GEN>, bool_constant<MASK>) names the instantiation.
    template <typename K>
    int launch(int rows_f64, int rows_f32, const char* name, void* stream, K&& kernel_of) const
    {
        const int JT = ft == TPG_F64 ? rows_f64 : rows_f32;
        const long long tiles = (g.Ny + JT - 1) / JT;
        if (tiles * (g.Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("momentum advection: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
        const MomentumPtrs p = pointers();
        void* all[13];
        const int na = arrays(all);
        hipStream_t st = tpg::as_stream(stream);
        return dispatch_ft(ft, [&](auto ty) {
            typedef decltype(ty) T;
            const ChunkPlan cp = chunk_plan<T>(g, all, na);
            const int cpr = g.Nx / cp.W;
            const MomentumArgs a{ g.Nx, g.Ny, g.Nz, g.sx, cpr, (int)(tiles * cpr), g.plane, interior2(g), interior3(g), n_fc ? (double)(T)mask_value : 0.0 };
            const unsigned blocks = (unsigned)((a.items + 255) / 256);
            dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
                auto go = [&](auto mask) {
                    void (*const kernel)(MomentumPtrs, MomentumArgs) = kernel_of(ty, cw, gen, mask);
                    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, p, a);
                };
                if (n_fc) go(std::true_type{});
                else      go(std::false_type{});
            });
            return tpg::launch_status(name);
        });
    }
};

}  // namespace
