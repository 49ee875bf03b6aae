// tpg_weno_vs.hip -- the vector-invariant advection tendency of the horizontal velocities of the drivers' scheme,
// WENOVectorInvariant(vorticity_order = 5), Gu at (Face, Center, Center) and Gv at (Center, Face, Center), for gfx950
// (tpg_weno_vs_momentum_advection_tendency): tpg_weno_vi_momentum_advection_tendency (tpg_weno_vi.hip) with the smoothness of the WENO5
// vorticity reconstruction measured on the velocities (VelocityStencil) instead of on the vorticity itself (DefaultStencil).
// [recalled: Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = VelocityStencil(), vertical_scheme =
// WENO(order = 5), kinetic_energy_gradient_scheme = WENO(order = 5), divergence_scheme = WENO(order = 5), upwinding =
// OnlySelfUpwinding(cross_scheme = WENO(order = 5))); biased WENO weights for VelocityStencil -- the smoothness indicators of the
// tangential stencils of the two velocities averaged onto (Face, Face), summed and halved (beta_sum); parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_weno_vs.h: include/tripolar_hip_weno_vi.h's with zr replaced.  Evaluated in the
// field type T with no contraction; every operation is one correctly rounded IEEE operation.  Hx, Hy >= 3, Hz >= 1; only interior cells of
// Gu, Gv are written.
//
// TWO launches on the caller's stream, as in tpg_weno_vi.hip:
// 1. k_weno_momentum_advection in its vorticity-only form with SW::VS (tpg_weno_vorticity_kernel.hpp, the one definition) leaves hu in Gu
//    and hv in Gv: W5V (weno_face_vs, tpg_weno_face.hpp) of the Z window and the windows of UB and VB at the same nodes.  2 rows per item in
//    both precisions; Z beside a chunk from the neighbouring lanes, UB and VB beside it from element loads (chosen by measurement, like the
//    rows: profiles/weno_vs/, with the registers).
// 2. k_weno_vi_finish (tpg_weno_vi_finish_kernel.hpp, the one definition, shared with tpg_weno_vi.hip), unchanged.
// The FULL form with this stencil (the centred vertical term with VelocityStencil) is not built: nobody's scheme needs it.
// No scratch, no LDS, no atomics, nothing allocated, no host wait; element offsets are 64-bit.
#include "tpg_momentum_tendency.hpp"
#include "tpg_weno_face.hpp"
#include "tpg_weno_vorticity_kernel.hpp"
#include "tpg_weno_vi_finish_kernel.hpp"
#include "../../include/tripolar_hip_weno_vs.h"

// compile-time switches of the A/B in profiles/weno_vs/ (make WENO_VS_TAG=_lanes WENO_VS_FLAGS=-DTPG_WVS_SHARE=1)
#ifndef TPG_WVS_SHARE
#define TPG_WVS_SHARE 0
#endif
#ifndef TPG_WVS_JT
#define TPG_WVS_JT 2
#endif
#ifndef TPG_WVS_JT_F32
#define TPG_WVS_JT_F32 2
#endif
#ifndef TPG_WVS_NT
#define TPG_WVS_NT 1
#endif

namespace {

constexpr bool NT = TPG_WVS_NT;            // Gu, Gv go out in streaming stores
constexpr int VROWS = TPG_WVS_JT;          // rows per item of the first launch, Float64
constexpr int VROWS_F32 = TPG_WVS_JT_F32;  // and Float32
struct VelocityStencilSwitches {           // of the first launch: neighbour-lane Z, ONE wave per SIMD, VelocityStencil smoothness
    static constexpr bool SHARE = true;
    static constexpr bool NT = TPG_WVS_NT;
    static constexpr int WAVES = 1;
    static constexpr bool VS = true;
    static constexpr bool SHARE_VS = TPG_WVS_SHARE;                // true: UB, VB beside the chunk come from the neighbouring lanes, as Z does.
                                                                   // Built false: every lane forms them from element loads, 5 % / 3 % faster
};

template <typename T>
constexpr int rows_of() { return sizeof(T) == 8 ? VROWS : VROWS_F32; }

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_weno_vs_last_error(void) { return tpg_last_error(); }

int tpg_weno_vs_momentum_advection_tendency(const void* u, const void* v, const void* w, void* Gu, void* Gv, const void* dx_fc, const void* dy_fc,
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
    if (int rc = call.launch(VROWS, VROWS_F32, "k_weno_momentum_advection (vorticity term, VelocityStencil)", stream, [](auto ty, auto cw, auto gen, auto) {
            return k_weno_momentum_advection<decltype(ty), decltype(cw)::value, decltype(gen)::value, false, rows_of<decltype(ty)>(), 0, VelocityStencilSwitches, false>;
        })) return rc;
    return call.launch(1, 1, "k_weno_vi_finish", stream, [](auto ty, auto cw, auto gen, auto mask) {
        return k_weno_vi_finish<decltype(ty), decltype(cw)::value, decltype(gen)::value, decltype(mask)::value, NT>;
    });
}

}  // extern "C"
