// tpg_weno_momentum.hip -- the vector-invariant advection tendency of the horizontal velocities with the WENO5-upwinded vorticity term, Gu at
// (Face, Center, Center) and Gv at (Center, Face, Center), for gfx950 (tpg_weno_momentum_advection_tendency): the momentum half of the scheme
// the reference's drivers build, and like tpg_momentum_advection_tendency's result the Gu, Gv of the AB2 step of the velocities.
// [recalled: Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(), vertical_scheme =
// EnergyConserving()); parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_weno_momentum.h: everything is tpg_momentum_advection_tendency's (tpg_momentum.hip: Z, P,
// Q, K, A, S, R, vh, uh, bu, bv, vu, vv, the mask, the order of evaluation) but the vorticity term.  Hx, Hy >= 3, Hz >= 1; only interior cells
// of Gu, Gv are written.
//
// ONE launch for both fields: k_weno_momentum_advection in its FULL form.  The kernel, what Z costs, the wave edges and the resources are in
// tpg_weno_vorticity_kernel.hpp, which tpg_weno_vi.hip includes too; this file holds the library's compile-time switches and its entry point.
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_weno_vorticity_kernel.hpp"
#include "../../include/tripolar_hip_weno_momentum.h"

// compile-time switches of the A/B in profiles/weno_momentum/ (make WENO_MOMENTUM_TAG=_jt1 WENO_MOMENTUM_FLAGS=-DTPG_WMOM_JT=1,
// -DTPG_WMOM_JT_F32=1, -DTPG_WMOM_LOOKAHEAD=0, -DTPG_WMOM_LOOKAHEAD_F32=2, -DTPG_WMOM_SHARE=0, -DTPG_WMOM_NT=0 or -DTPG_WMOM_WAVES=2).
#ifndef TPG_WMOM_JT
#define TPG_WMOM_JT 2
#endif
#ifndef TPG_WMOM_JT_F32
#define TPG_WMOM_JT_F32 2
#endif
#ifndef TPG_WMOM_LOOKAHEAD
#define TPG_WMOM_LOOKAHEAD 0
#endif
#ifndef TPG_WMOM_LOOKAHEAD_F32
#define TPG_WMOM_LOOKAHEAD_F32 0
#endif
#ifndef TPG_WMOM_SHARE
#define TPG_WMOM_SHARE 1
#endif
#ifndef TPG_WMOM_NT
#define TPG_WMOM_NT 1
#endif
#ifndef TPG_WMOM_WAVES
#define TPG_WMOM_WAVES 1
#endif

namespace {

template <typename T> constexpr int ROWS = sizeof(T) == 8 ? TPG_WMOM_JT : TPG_WMOM_JT_F32;                   // rows per work item
template <typename T> constexpr int LOOKAHEAD = sizeof(T) == 8 ? TPG_WMOM_LOOKAHEAD : TPG_WMOM_LOOKAHEAD_F32;   // levels whose loads are in flight (0: no ring)
struct Switches {
    static constexpr bool SHARE = TPG_WMOM_SHARE;   // the Z beside the chunk come from the neighbouring lanes
    static constexpr bool NT = TPG_WMOM_NT;         // Gu, Gv go out in streaming stores
    static constexpr int WAVES = TPG_WMOM_WAVES;    // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)
    static constexpr bool VS = false;               // DefaultStencil smoothness: the built rule
};

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_weno_momentum_last_error(void) { return tpg_last_error(); }

int tpg_weno_momentum_advection_tendency(const void* u, const void* v, const void* w, void* Gu, void* Gv, const void* dx_fc, const void* dy_fc,
                                         const void* az_fc, const void* dx_cf, const void* dy_cf, const void* az_cf, const void* az_cc,
                                         const void* az_ff, const void* dz_f, const int32_t* n_fc, const int32_t* n_cf, double mask_value,
                                         int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    const MomentumCall call{ u, v, w, Gu, Gv, dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_f, n_fc, n_cf, mask_value,
                             tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft };
    if (int rc = call.check(HALO, "Z[i, j-2..j+3] and Z[i-2..i+3, j], that is u, v[i-3..i+3, j-3..j+3, k-1..k+1], and w[i-1, j], w[i, j-1]")) return rc;
    return call.launch(ROWS<double>, ROWS<float>, "k_weno_momentum_advection", stream, [](auto ty, auto cw, auto gen, auto mask) {
        typedef decltype(ty) T;
        return k_weno_momentum_advection<T, decltype(cw)::value, decltype(gen)::value, decltype(mask)::value, ROWS<T>, LOOKAHEAD<T>, Switches, true>;
    });
}

}  // extern "C"
