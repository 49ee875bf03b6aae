// tpg_weno_xyz.hip -- the flux-form advection tendency of the tracers at (Center, Center, Center) with a fifth-order WENO reconstruction in
// x, y AND z, for gfx950 (tpg_weno_xyz_tracer_advection_tendency): the scheme `WENO()` of the reference's distributed driver, and like
// tpg_weno_tracer_advection_tendency's result the Gn of the AB2 step of the tracers.
// [recalled: Oceananigans' WENO() = FluxFormAdvection(WENO(order = 5) x3) on a z-Bounded grid; parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_weno_xyz.h: x and y are include/tripolar_hip_weno.h's (R5 = weno_face of
// tpg_weno_face.hpp, five selects and ONE evaluation per face); a z-face takes the centred mean at the two walls, the upwind cell one face
// away from a wall, R3 (weno_face3) two faces away and R5 from three on, whichever way the flow goes.  Evaluated in the field type T, in
// exactly that order, with no contraction; every operation is one correctly rounded IEEE operation.
// - Cells read: c[-2..Nx+3, j, k], c[i, -2..Ny+3, k], c[i, j, 0..Nz+1] (no corner halo cell, no z-halo plane but 0 and Nz + 1 at any Hz);
//   u[1..Nx+1, j, k], v[i, 1..Ny+1, k], w[i, j, 1..Nz+1]; the same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.
// - Only interior cells of G are written.  Mask and several tracers: as in tpg_weno_tracer_advection_tendency.
//
// The kernel is k_weno_tracer_advection in its ZW form, one tracer per item (grid.y counts the tracers), a level's loads going out at the
// level.  The kernel, the z-window, what it costs in registers and the launch are in tpg_weno_tracer_kernel.hpp, which tpg_weno.hip
// includes too; this file holds the library's compile-time switches and its entry point.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_weno_tracer_kernel.hpp"
#include "../../include/tripolar_hip_weno_xyz.h"

// compile-time switches of the A/B in profiles/weno_xyz/ (make WENO_XYZ_TAG=_jt2w1 WENO_XYZ_FLAGS='-DTPG_WXYZ_JT=2 -DTPG_WXYZ_WAVES=1',
// -DTPG_WXYZ_SHARE=0 or -DTPG_WXYZ_NT=0).  What was measured at 3600 x 1800 x 75 and why these are the defaults: DESIGN.md 6, profiles/weno_xyz/.
#ifndef TPG_WXYZ_JT
#define TPG_WXYZ_JT 2
#endif
#ifndef TPG_WXYZ_WAVES
#define TPG_WXYZ_WAVES 1
#endif
#ifndef TPG_WXYZ_SHARE
#define TPG_WXYZ_SHARE 1
#endif
#ifndef TPG_WXYZ_NT
#define TPG_WXYZ_NT 1
#endif

namespace {

struct Switches {
    static constexpr int JT = TPG_WXYZ_JT;               // rows per work item
    static constexpr int WAVES = TPG_WXYZ_WAVES;         // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)
    static constexpr bool SHARE_X = TPG_WXYZ_SHARE;      // the east-most x-flux of an item comes from the lane to the east (where Hx >= W)
    static constexpr bool NT = TPG_WXYZ_NT;              // G goes out in streaming stores
    static constexpr int GROUP = 1, LOOKAHEAD = 0;       // the z-window: one tracer per item, no ring (not switches)
};

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_weno_xyz_last_error(void) { return tpg_last_error(); }

int tpg_weno_xyz_tracer_advection_tendency(const void* const* c, void* const* G, int nfields, const void* u, const void* v, const void* w,
                                           const void* dy_fc, const void* dx_cf, const void* az_cc, const void* dz_c, const int32_t* n_cc,
                                           double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    const TracerCall call{ c, G, nfields, u, v, w, dy_fc, dx_cf, az_cc, dz_c, n_cc, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft };
    if (int rc = call.check(HALO, 1, "c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1]")) return rc;
    return launch_weno_tracers<true, Switches>(call, mask_value, "k_weno_xyz_tracer_advection", stream);
}

}  // extern "C"
