/*
 * tripolar_hip_weno_vs.h -- C ABI of libtripolar_hip_weno_vs.so: the vector-invariant advection tendency of the horizontal velocities of
 * the drivers' scheme, WENOVectorInvariant(vorticity_order = 5), on the fields of a TripolarGrid for MI355X (gfx950), beside
 * libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word: extern "C", plain pointers, caller-owned DEVICE
 * memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a positive
 * hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, the thirteenth, as the other operator libraries are: the export lists of the other twelve are pinned, and
 * tpg_weno_vi_momentum_advection_tendency (include/tripolar_hip_weno_vi.h) keeps its rule and its refusals.  The libraries share no state:
 * tpg_weno_vs_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on this thread; status codes
 * and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_WENO_VS_H
#define TRIPOLAR_HIP_WENO_VS_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_weno_vs_last_error(void);

/* ---- the velocity tendencies with upwinding in every term and VelocityStencil smoothness of the vorticity reconstruction -------------------
 * The scheme is Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = VelocityStencil(), vertical_scheme =
 * WENO(order = 5), kinetic_energy_gradient_scheme = WENO(order = 5), divergence_scheme = WENO(order = 5), upwinding =
 * OnlySelfUpwinding(cross_scheme = WENO(order = 5))): the drivers' WENOVectorInvariant(vorticity_order = 5).  The weights of the WENO5
 * reconstruction of the vorticity are measured on the two velocities, not on the vorticity itself: a smooth velocity with a rough
 * vorticity is reconstructed at the full linear order.  The results are the `Gu`, `Gv` of tpg_ab2_step_velocities
 * (include/tripolar_hip_timestep.h).
 * [recalled: Oceananigans' biased WENO weights for VelocityStencil -- the smoothness indicators of the tangential stencils of
 * u averaged in y and v averaged in x onto (Face, Face), summed and halved (beta_sum); parity unpinned, like every operator here]
 *
 * THE RULE.  Everything not named here is include/tripolar_hip_weno_vi.h's, bit for bit: Z, vhat, uhat, the selection, vu, bu, vvert, bv,
 * the mask, the arrays, the refusals and the order of evaluation.  Every operation is one correctly rounded IEEE operation in the field
 * type T, with no contraction.  Only zr inside hu and hv is replaced.
 *
 *   UB[i,j,k] = T(0.5) * (u[i,j-1,k] + u[i,j,k])        u averaged in y onto (Face, Face)
 *   VB[i,j,k] = T(0.5) * (v[i-1,j,k] + v[i,j,k])        v averaged in x onto (Face, Face)
 *
 *   W5V(q0..q4; a0..a4; b0..b4) = R(q0..q4) of include/tripolar_hip_weno.h with one change:
 *       p2, p1, p0 from q0..q4 as in R;
 *       bA_s = K(13,12) * (sA_s * sA_s) + T(0.25) * (dA_s * dA_s)   with s_s, d_s formed from a0..a4 exactly as R forms them from q
 *       bB_s = the same from b0..b4
 *       b_s  = T(0.5) * (bA_s + bB_s)                      s = 2, 1, 0
 *       tau, r_s, a_s and the quotient as in R, from these b_s.
 *
 *   u: zr = vhat >= 0 ? W5V(Z[i, j-2..j+2]; UB[i, j-2..j+2]; VB[i, j-2..j+2])
 *                     : W5V(Z[i, j+3..j-1]; UB[i, j+3..j-1]; VB[i, j+3..j-1])
 *      hu = -(vhat * zr)
 *   v: zr = uhat >= 0 ? W5V(Z[i-2..i+2, j]; UB[i-2..i+2, j]; VB[i-2..i+2, j])
 *                     : W5V(Z[i+3..i-1, j]; UB[i+3..i-1, j]; VB[i+3..i-1, j])
 *      hv = uhat * zr
 *   Gu = -((hu + vu) + bu),  Gv = -((hv + vvert) + bv)      as in the weno_vi header
 *
 * - Selection.  The fifteen inputs of a W5V are selected and it is evaluated once per node and direction.  `>= 0` is true for -0 and
 *   false for NaN.
 * - Degeneration.  W5V(q; q; q) is R(q) bit for bit for finite inputs whose indicators neither overflow nor go subnormal: x + x and
 *   T(0.5) * (2x) are exact there.
 * - Cells read are unchanged.  UB[i, j-2..j+3] reads u at (0, -3..+3); VB[i, j-2..j+3] reads v at (-1..0, -2..+3); UB[i-2..i+3, j] reads u
 *   at (-2..+3, -1..0); VB[i-2..i+3, j] reads v at (-3..+3, 0).  All of these are in the weno_vi header's list already -- they are the
 *   cells of u and v the Z of the same windows read -- so: halo (3, 3, 1), the same corner cells, the same metric cells.
 * - Non-finite values.  A non-finite u or v now also arrives through UB / VB at every node whose window holds it.  It arrives as NaN, via
 *   tau = |b0 - b2|.
 * - One definition each.  UB, VB and W5V each have one definition, so a value formed again at a chunk's edge has the same bits.
 * - Stays out.  The centred vertical term with this stencil (tpg_weno_momentum_advection_tendency keeps DefaultStencil); Oceananigans'
 *   drop of the order beside the south wall and immersed nodes; stretched-grid coefficients; other orders.
 *
 * Arrays, alignment, the TWO launches on `stream` (the first leaves hu, hv in Gu, Gv), 64-bit element offsets, capture into a HIP graph:
 * tpg_weno_vi_momentum_advection_tendency's, argument for argument, dz_c (Nz values) included.
 *
 * Refusals, in this order, each with its own message (tpg_weno_vi_momentum_advection_tendency's, word for word):
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. null u, v or w, then null Gu or Gv, then a null metric plane or dz_c: TPG_ERR_INVALID_ARGUMENT;
 *  3. one of n_fc, n_cf without the other: TPG_ERR_INVALID_ARGUMENT;
 *  4. a pointer off its element alignment, a count plane off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  5. Gu or Gv overlapping u, v, w (whose parent is one level longer) or each other: TPG_ERR_INVALID_ARGUMENT;
 *  6. Hx < 3, Hy < 3 or Hz < 1: TPG_ERR_UNSUPPORTED, the message names the stencil and the halo passed;
 *  7. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (4, 3, 1) at halo (3, 3, 1) and (4, 4, 5) at halo (4, 4, 4); a latitude band down to
 * Hy rows gives the rows of the global call. */
int tpg_weno_vs_momentum_advection_tendency(const void *u, const void *v, const void *w, void *Gu, void *Gv,
                                            const void *dx_fc, const void *dy_fc, const void *az_fc, const void *dx_cf, const void *dy_cf,
                                            const void *az_cf, const void *az_cc, const void *az_ff, const void *dz_c, const int32_t *n_fc,
                                            const int32_t *n_cf, double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                                            int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_WENO_VS_H */
