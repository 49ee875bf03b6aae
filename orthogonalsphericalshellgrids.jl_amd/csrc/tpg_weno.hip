// tpg_weno.hip -- the flux-form advection tendency of the tracers at (Center, Center, Center) with a fifth-order WENO reconstruction in x
// and y and the centred mean in z, for gfx950 (tpg_weno_tracer_advection_tendency): the scheme of the reference's drivers, and like
// tpg_tracer_advection_tendency's result the Gn of the AB2 step of the tracers.
// [recalled: Oceananigans' FluxFormAdvection(WENO(order = 5), WENO(order = 5), Centered()), uniform-grid coefficients, Jiang-Shu smoothness
// indicators, WENO-Z weights, eps = 1e-8; parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_weno.h: R(q0..q4) (weno_face of tpg_weno_face.hpp, operation for operation), the selection
// Mx >= 0 ? R(c[i-3..i+1]) : R(c[i+2..i-2]) (upwind_flux: five selects, ONE evaluation of R per face), Mx, My, Mz, V, Fz and the last
// line those of tpg_tracer_advection_tendency.  Evaluated in the field type T, in exactly that order, with no contraction; every operation
// is one correctly rounded IEEE operation.  Each flux is formed once; where one is formed twice (tile edges) it has the same bits.
// - Cells read: c[-2..Nx+3, j, k], c[i, -2..Ny+3, k], c[i, j, 0..Nz+1] (a plus-shaped stencil, no corner halo cell); u[1..Nx+1, j, k],
//   v[i, 1..Ny+1, k], w[i, j, 1..Nz+1]; the same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.  So Hx >= 3, Hy >= 3, Hz >= 1.
// - Only interior cells of G are written.  Mask and several tracers: as in tpg_tracer_advection_tendency.
//
// The kernel is k_weno_tracer_advection in its x-y form.  The kernel, its work item, the SHARE form of the x-flux, the registers and the
// launch are in tpg_weno_tracer_kernel.hpp, which tpg_weno_xyz.hip includes too; this file holds the library's compile-time switches and
// its entry point.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_weno_tracer_kernel.hpp"
#include "../../include/tripolar_hip_weno.h"

// compile-time switches of the A/B in profiles/weno/ (make WENO_TAG=_jt1 WENO_FLAGS=-DTPG_WENO_JT=1, -DTPG_WENO_SHARE=0, -DTPG_WENO_TG=2,
// -DTPG_WENO_LOOKAHEAD=1, -DTPG_WENO_NT=0 or -DTPG_WENO_WAVES=1).  What was measured at 3600 x 1800 x 75 and why these are the defaults:
// DESIGN.md 6, profiles/weno/.
#ifndef TPG_WENO_TG
#define TPG_WENO_TG 1
#endif
#ifndef TPG_WENO_JT
#define TPG_WENO_JT 2
#endif
#ifndef TPG_WENO_SHARE
#define TPG_WENO_SHARE 1
#endif
#ifndef TPG_WENO_LOOKAHEAD
#define TPG_WENO_LOOKAHEAD 0
#endif
#ifndef TPG_WENO_NT
#define TPG_WENO_NT 1
#endif
#ifndef TPG_WENO_WAVES
#define TPG_WENO_WAVES 2
#endif

namespace {

struct Switches {
    static constexpr int GROUP = TPG_WENO_TG;            // the largest group of tracers a work item takes, sharing Mx, My, Mz: 1 (no grouped kernel), 2 or 4
    static constexpr int JT = TPG_WENO_JT;               // rows per work item
    static constexpr bool SHARE_X = TPG_WENO_SHARE;      // the east-most x-flux of an item comes from the lane to the east (where Hx >= W)
    static constexpr int LOOKAHEAD = TPG_WENO_LOOKAHEAD; // levels whose loads are in flight ahead of the arithmetic (0: no ring)
    static constexpr bool NT = TPG_WENO_NT;              // G goes out in streaming stores
    static constexpr int WAVES = TPG_WENO_WAVES;         // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)
};

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_weno_last_error(void) { return tpg_last_error(); }

int tpg_weno_tracer_advection_tendency(const void* const* c, void* const* G, int nfields, const void* u, const void* v, const void* w,
                                       const void* dy_fc, const void* dx_cf, const void* az_cc, const void* dz_c, const int32_t* n_cc,
                                       double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    const TracerCall call{ c, G, nfields, u, v, w, dy_fc, dx_cf, az_cc, dz_c, n_cc, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft };
    if (int rc = call.check(HALO, 1, "c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-1..k+1]")) return rc;
    return launch_weno_tracers<false, Switches>(call, mask_value, "k_weno_tracer_advection", stream);
}

}  // extern "C"
