/*
 * tripolar_hip_weno_momentum.h -- C ABI of libtripolar_hip_weno_momentum.so: the vector-invariant advection tendency of the horizontal
 * velocities with the WENO5-upwinded vorticity term on the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so
 * (include/tripolar_hip.h), whose conventions hold here word for word: extern "C", plain pointers, caller-owned DEVICE memory, padded parent
 * arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous
 * on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, the tenth, as the other operator libraries are: the export lists of the other nine are pinned.  The libraries
 * share no state: tpg_weno_momentum_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on this
 * thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_WENO_MOMENTUM_H
#define TRIPOLAR_HIP_WENO_MOMENTUM_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_weno_momentum_last_error(void);

/* ---- the velocity tendencies with the upwinded vorticity flux ------------------------------------------------------------------------------
 * The scheme is Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(),
 * vertical_scheme = EnergyConserving()): the vorticity term of tpg_momentum_advection_tendency (include/tripolar_hip_momentum.h) with the
 * vertical vorticity reconstructed by fifth-order WENO against the transverse velocity; the vertical term and the kinetic-energy gradient
 * are that call's.  The results are the `Gu`, `Gv` of tpg_ab2_step_velocities (include/tripolar_hip_timestep.h).
 * [recalled: Oceananigans' horizontal_advection_U / horizontal_advection_V for VectorInvariant with a WENO vorticity scheme and
 * DefaultStencil smoothness: the vorticity reconstructed in y at (Face, Center) against the transverse velocity v over dx, in x at
 * (Center, Face) against u over dy; uniform-grid coefficients, Jiang-Shu smoothness indicators, WENO-Z weights, eps = 1e-8; parity
 * unpinned, like every operator here]
 *
 * THE RULE.  Everything not named here is include/tripolar_hip_momentum.h's, with the same bits: Z, P, Q, K, A, S, R, vh, uh, bu, bv, vu,
 * vv, the mask, the arrays and the order of evaluation.  Every operation is one correctly rounded IEEE operation in the field type T.
 * There is no contraction.  W5(q0, q1, q2, q3, q4) is R(q0, q1, q2, q3, q4) of include/tripolar_hip_weno.h, the same bits: q2 is the
 * upwind value and q3 the downwind one (the name differs because R is taken in the momentum rule).
 *
 *  u: vhat = vh / dx_fc[i,j]
 *     zr   = vhat >= 0 ? W5(Z[i,j-2], Z[i,j-1], Z[i,j],   Z[i,j+1], Z[i,j+2])
 *                      : W5(Z[i,j+3], Z[i,j+2], Z[i,j+1], Z[i,j],   Z[i,j-1])         (all at i, k)
 *     hu   = -(vhat * zr)
 *     Gu[i,j,k] = -((hu + vu) + bu)
 *
 *  v: uhat = uh / dy_cf[i,j]
 *     zr   = uhat >= 0 ? W5(Z[i-2,j], Z[i-1,j], Z[i,j],   Z[i+1,j], Z[i+2,j])
 *                      : W5(Z[i+3,j], Z[i+2,j], Z[i+1,j], Z[i,j],   Z[i-1,j])         (all at j, k)
 *     hv   = uhat * zr
 *     Gv[i,j,k] = -((hv + vv) + bv)
 *
 * - Selection.  `>= 0` is true for -0 and false for NaN, as in the tracer rule.  Five inputs are selected, and W5 is evaluated once per
 *   node and direction.
 * - Shared quantities.  Z has one definition.  An item that recomputes a Z its neighbour also forms gets the same bits.
 * - Cells read, relative to the node, over the interior.  Z is needed at (0, -2..+3) and (-2..+3, 0).  Beside the momentum rule's own
 *   cells (u at {(0,0), (+-1,0), (0,+-1), (1,-1)} and k+-1 at (0,0); v at {(0,0), (+-1,0), (0,+-1), (-1,1)} and k+-1 at (0,0); w at faces
 *   k, k+1 at {(0,0), (-1,0), (0,-1)}), u is read at (0, -3..+3) and (-2..+3, -1..0), v at (-1..0, -2..+3) and (-3..+3, 0): two crosses,
 *   not a box.  Corner halo cells ARE read (u[Nx+3, 0], v[0, -1], v[0, Ny+3]).  The momentum rule's cells u(1,-1) and v(-1,1) stay (vh
 *   and uh read them through K).  Metric planes: dx_fc at (0, -3..+3) and (-2..+3, -1..0); dy_cf at (-1..0, -2..+3) and (-3..+3, 0);
 *   az_ff at (0, -2..+3) and (-2..+3, 0); dx_cf at {(0,0), (-1,0), (0,1), (-1,1)}; dy_fc at {(0,0), (1,0), (0,-1), (1,-1)}; az_cc at
 *   {(0,0), (-1,0), (0,-1)}; az_fc and az_cf at (0,0).
 * - Halos.  Hx >= 3, Hy >= 3, Hz >= 1.  The caller has filled every halo of u and v and the horizontal halos of w.  The rows Ny+1..Ny+3
 *   are the Zipper's, the rows -2..0 what the south condition left there.
 * - Written.  Only interior cells of Gu and Gv.
 * - Non-finite Z.  A zero divisor divides: az_ff is zero at the grid poles, and Z there is Inf or NaN.  In the momentum rule such a Z
 *   reaches the two Gu and the two Gv nodes beside it.  Here it reaches EVERY node whose window holds it: the six Gu nodes
 *   (i, j-3..j+2) and the six Gv nodes (i-3..i+2, j) of a non-finite Z[i,j] (five of each for a given sign of the transverse velocity),
 *   through the smoothness indicators as NaN.  A model masks them.
 * - Mask, dz_f, signs, zero divisors: as in include/tripolar_hip_momentum.h.
 *
 * Arrays: as in include/tripolar_hip_momentum.h.  Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows
 * and pointers sit on the 16-B grid, element-aligned chunks otherwise; ONE launch for both fields; no atomics, no LDS, nothing allocated,
 * asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element offsets are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message (tpg_momentum_advection_tendency's, without its scheme item):
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. null u, v or w, then null Gu or Gv, then a null metric plane or dz_f: TPG_ERR_INVALID_ARGUMENT;
 *  3. one of n_fc, n_cf without the other: TPG_ERR_INVALID_ARGUMENT;
 *  4. a pointer off its element alignment, a count plane off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  5. Gu or Gv overlapping u, v, w (whose parent is one level longer) or each other: TPG_ERR_INVALID_ARGUMENT;
 *  6. Hx < 3, Hy < 3 or Hz < 1: TPG_ERR_UNSUPPORTED, the message names the stencil and the halo passed;
 *  7. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (4, 3, 1) at halo (3, 3, 1) -- Nx = Hx + 1, Ny = Hy: the arms end on the last halo
 * cell -- and (4, 4, 5) at halo (4, 4, 4), and up past 2^31 elements a parent (8640 x 4320 x 64 at halo 4, with n_fc, n_cf); a latitude
 * band down to Hy rows gives the rows of the global call (tests/test_gpu_tendency_edges.py). */
int tpg_weno_momentum_advection_tendency(const void *u, const void *v, const void *w, void *Gu, void *Gv,
                                         const void *dx_fc, const void *dy_fc, const void *az_fc, const void *dx_cf, const void *dy_cf,
                                         const void *az_cf, const void *az_cc, const void *az_ff, const void *dz_f, const int32_t *n_fc,
                                         const int32_t *n_cf, double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                                         int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_WENO_MOMENTUM_H */
