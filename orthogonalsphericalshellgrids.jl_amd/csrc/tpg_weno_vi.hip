// tpg_weno_vi.hip -- the vector-invariant advection tendency of the horizontal velocities with upwinding in every term, Gu at
// (Face, Center, Center) and Gv at (Center, Face, Center), for gfx950 (tpg_weno_vi_momentum_advection_tendency): the WENO5-upwinded vorticity
// flux of tpg_weno_momentum_advection_tendency, the upwinded vertical term (the divergence upwinded against the advected velocity, the
// WENO flux of u and v in z) and the upwinded kinetic-energy gradient.  Only the smoothness stencil of the vorticity reconstruction
// (DefaultStencil here) separates it from the drivers' WENOVectorInvariant(vorticity_order = 5).
// [recalled: Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(), vertical_scheme =
// WENO(order = 5), kinetic_energy_gradient_scheme = WENO(order = 5), divergence_scheme = WENO(order = 5), upwinding =
// OnlySelfUpwinding(cross_scheme = WENO(order = 5))); parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_weno_vi.h.  Evaluated in the field type T with no contraction; every operation is
// one correctly rounded IEEE operation.  Hx, Hy >= 3, Hz >= 1; only interior cells of Gu, Gv are written.
//
// TWO launches on the caller's stream, the split form (profiles/weno_vi/README.md has the register figures behind the choice):
// 1. k_weno_momentum_advection in its vorticity-only form (tpg_weno_vorticity_kernel.hpp, the one definition, shared with
//    tpg_weno_momentum.hip) leaves hu in Gu and hv in Gv: 2 rows per item in both precisions, no look-ahead ring, the Z beside a chunk from
//    the neighbouring lanes.
// 2. k_weno_vi_finish (tpg_weno_vi_finish_kernel.hpp, the one definition, shared with tpg_weno_vs.hip) reads hu, hv back at its own nodes and stores -((hu + vu) + bu), -((hv + vvert) + bv), masked: the order of the three
//    additions is the rule's, so the bits are those of one evaluation.  An item is ONE chunk of W columns of ONE row and walks all levels.
//    It loads once and keeps in registers the cells of dy_fc, dx_cf, az_cc, dx_fc, dy_cf, az_fc and az_cf its nodes read, and the counts.
//    It carries from level to level the z-windows of u and v on its columns (five levels; the sixth arrives with the level) and FZu, FZv at
//    the level's bottom face.  Per level: the row of u from three columns west to three east of the chunk, the rows -3 .. +2 of u on the
//    columns 0 .. W, the mirror image of v, w at the top face two cells out, and hu, hv.  The order of a z-face is the same in every lane:
//    a scalar branch, as in the ZW form of k_weno_tracer_advection.  Every DU, DV, DKU of the neighbouring chunks is formed by the item itself from
//    element loads (the same bits); taking them from the neighbouring lanes is not built.
// No load leaves the cells the header lists: the levels the z-window loads ahead of a face of reduced order are clamped onto the planes
// 0 .. Nz + 1 and never selected.  Gu, Gv go out as streaming stores in both launches.
//
// Resources (gfx950 code object metadata of the build, profiles/weno_vi/resources.json): no scratch, no LDS in any instantiation;
// __launch_bounds__(256, 1), ONE wave per SIMD, like k_weno_momentum_advection.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_momentum_tendency.hpp"
#include "tpg_weno_face.hpp"
#include "tpg_weno_vorticity_kernel.hpp"
#include "tpg_weno_vi_finish_kernel.hpp"
#include "../../include/tripolar_hip_weno_vi.h"

// compile-time switch of the A/B in profiles/weno_vi/ (make WENO_VI_TAG=_nt0 WENO_VI_FLAGS=-DTPG_WVI_NT=0)
#ifndef TPG_WVI_NT
#define TPG_WVI_NT 1
#endif

namespace {

constexpr bool NT = TPG_WVI_NT;            // Gu, Gv go out in streaming stores
constexpr int VROWS = 2;                   // rows per item of the first launch
struct VorticitySwitches {                 // of the first launch: neighbour-lane Z, ONE wave per SIMD
    static constexpr bool SHARE = true;
    static constexpr bool NT = TPG_WVI_NT;
    static constexpr int WAVES = 1;
    static constexpr bool VS = false;          // DefaultStencil smoothness: the built rule
};

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_weno_vi_last_error(void) { return tpg_last_error(); }

int tpg_weno_vi_momentum_advection_tendency(const void* u, const void* v, const void* w, void* Gu, void* Gv, const void* dx_fc, const void* dy_fc,
                                            const void* az_fc, const void* dx_cf, const void* dy_cf, const void* az_cf, const void* az_cc,
                                            const void* az_ff, const void* dz_c, const int32_t* n_fc, const int32_t* n_cf, double mask_value,
                                            int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    const MomentumCall call{ u, v, w, Gu, Gv, dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_c, n_fc, n_cf, mask_value,
                             tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft, "dz_c" };
    if (int rc = call.check(HALO, "u, v[i-3..i+3, j-3..j+3, k-3..k+3 within 0..Nz+1] and w[i-2..i+1, j], w[i, j-2..j+1]")) return rc;
    // every check precedes any launch: the second launch has the more items (one row each), so its bound is checked before the first
    if ((long long)Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("momentum advection: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }
    if (int rc = call.launch(VROWS, VROWS, "k_weno_momentum_advection (vorticity term)", stream, [](auto ty, auto cw, auto gen, auto) {
            return k_weno_momentum_advection<decltype(ty), decltype(cw)::value, decltype(gen)::value, false, VROWS, 0, VorticitySwitches, false>;
        })) return rc;
    return call.launch(1, 1, "k_weno_vi_finish", stream, [](auto ty, auto cw, auto gen, auto mask) {
        return k_weno_vi_finish<decltype(ty), decltype(cw)::value, decltype(gen)::value, decltype(mask)::value, NT>;
    });
}

}  // extern "C"
