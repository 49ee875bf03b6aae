/*
 * tripolar_hip_momentum.h -- C ABI of libtripolar_hip_momentum.so: the vector-invariant advection tendency of the horizontal velocities on
 * the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for
 * word: extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call
 * returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment
 * variable read.
 *
 * A library of its own, the eighth, as the other operator libraries are: the export lists of the other seven are pinned.  The libraries
 * share no state: tpg_momentum_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on this
 * thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_MOMENTUM_H
#define TRIPOLAR_HIP_MOMENTUM_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_momentum_last_error(void);

/* `scheme` of tpg_momentum_advection_tendency.  VectorInvariant()'s default is the only one built: the enstrophy-conserving vorticity term,
 * the energy-conserving vertical term and the kinetic-energy gradient.  Every other value is refused with TPG_ERR_UNSUPPORTED, the message
 * names it (the WENO5-upwinded vorticity term is a call of its own, include/tripolar_hip_weno_momentum.h; the energy-conserving scheme comes
 * later without an ABI change). */
#define TPG_MOMENTUM_ENSTROPHY_CONSERVING 0

/* ---- the velocity tendencies a hydrostatic model's AB2 step consumes ----------------------------------------------------------------------
 * With `buoyancy = nothing`, no Coriolis, no closure and no forcing, the whole 3-D tendency of u and v is minus U.grad(u), minus U.grad(v) in
 * vector-invariant form (the free-surface gradient is the sub-cycle's).  The results are the `Gu`, `Gv` of tpg_ab2_step_velocities
 * (include/tripolar_hip_timestep.h); `w` is what tpg_w_from_continuity (include/tripolar_hip_continuity.h) writes.
 * [recalled: Oceananigans' U_dot_grad_u / U_dot_grad_v for VectorInvariant() with EnstrophyConserving vorticity, the zeta2 w (Face, Center,
 * Face) / zeta1 w (Center, Face, Face) vertical terms and d/dx, d/dy of Kh at (Center, Center, Center); parity unpinned, like every
 * operator here]
 *
 * The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with
 * no contraction.  Every operation is one correctly rounded IEEE operation.  kf is a face index; w has Nz + 1 levels.
 *     Z[i,j,k]  = ((dy_cf[i,j] v[i,j,k] - dy_cf[i-1,j] v[i-1,j,k]) - (dx_fc[i,j] u[i,j,k] - dx_fc[i,j-1] u[i,j-1,k])) / az_ff[i,j]
 *                 (the vertical vorticity: tpg_vertical_vorticity's bits)
 *     P[i,j,k]  = dx_cf[i,j] * v[i,j,k]      Q[i,j,k] = dy_fc[i,j] * u[i,j,k]      A[i,j,kf] = az_cc[i,j] * w[i,j,kf]
 *     K[i,j,k]  = T(0.5) * (T(0.5) * (u[i,j,k]*u[i,j,k] + u[i+1,j,k]*u[i+1,j,k]) + T(0.5) * (v[i,j,k]*v[i,j,k] + v[i,j+1,k]*v[i,j+1,k]))
 *
 *  u: zb = T(0.5) * (Z[i,j,k] + Z[i,j+1,k])
 *     vh = T(0.5) * (T(0.5) * (P[i-1,j,k] + P[i-1,j+1,k]) + T(0.5) * (P[i,j,k] + P[i,j+1,k]))
 *     hu = -((zb * vh) / dx_fc[i,j])
 *     bu = (K[i,j,k] - K[i-1,j,k]) / dx_fc[i,j]
 *     S[i,j,kf] = (T(0.5) * (A[i-1,j,kf] + A[i,j,kf])) * ((u[i,j,kf] - u[i,j,kf-1]) / dz_f[kf])        kf = 1..Nz+1
 *     vu = (T(0.5) * (S[i,j,k] + S[i,j,k+1])) / az_fc[i,j]
 *     Gu[i,j,k] = -((hu + vu) + bu)
 *
 *  v: zb = T(0.5) * (Z[i,j,k] + Z[i+1,j,k])
 *     uh = T(0.5) * (T(0.5) * (Q[i,j-1,k] + Q[i+1,j-1,k]) + T(0.5) * (Q[i,j,k] + Q[i+1,j,k]))
 *     hv = (zb * uh) / dy_cf[i,j]
 *     bv = (K[i,j,k] - K[i,j-1,k]) / dy_cf[i,j]
 *     R[i,j,kf] = (T(0.5) * (A[i,j-1,kf] + A[i,j,kf])) * ((v[i,j,kf] - v[i,j,kf-1]) / dz_f[kf])
 *     vv = (T(0.5) * (R[i,j,k] + R[i,j,k+1])) / az_cf[i,j]
 *     Gv[i,j,k] = -((hv + vv) + bv)
 * - Shared quantities.  Each of Z, P, Q, K, A, S, R has one definition: forming it once or again at a tile edge gives the same bits.
 * - Signs.  Leading minus signs are sign flips.
 * - Zero divisors.  A zero divisor divides, as the rule says: the (Face, Center) / (Face, Face) nodes at the grid poles have zero metrics
 *   and give Inf / NaN.  A model masks them.
 * - dz_f.  Nz + 1 values in the field type: the centre-to-centre spacing at faces 1..Nz+1.  Faces 1 and Nz+1 use the halo centres.
 * - Cells read, relative to the node, over the interior.  u at (di,dj) in {(0,0), (+-1,0), (0,+-1), (1,-1)}, plus k+-1 at (0,0).
 *   v at {(0,0), (+-1,0), (0,+-1), (-1,1)}, plus k+-1 at (0,0).  w at faces k, k+1 at {(0,0), (-1,0), (0,-1)}.  Corner halo cells ARE read
 *   (u[Nx+1, 0], v[0, Ny+1]), and so are w's west column and south row.  dx_fc at {(0,0), (0,+-1), (1,0), (1,-1)}, dy_cf at
 *   {(0,0), (+-1,0), (0,1), (-1,1)}, az_ff at {(0,0), (0,1), (1,0)}, dx_cf at {(0,0), (-1,0), (0,1), (-1,1)}, dy_fc at
 *   {(0,0), (1,0), (0,-1), (1,-1)}, az_cc at {(0,0), (-1,0), (0,-1)}, az_fc and az_cf at (0,0).
 * - Halos.  Hx, Hy, Hz >= 1.  The caller has filled every halo of u and v and the horizontal halos of w.
 * - Written.  Only interior cells of Gu and Gv.
 * - Mask.  n_fc and n_cf, the (Face, Center) and (Center, Face) count planes (Ny x Nx int32, tpg_immersed_column_counts), are both given
 *   or both NULL.  With them, the nodes k <= min(max(n, 0), Nz) of Gu (by n_fc) and of Gv (by n_cf) hold T(mask_value) instead; everything
 *   is computed unmasked.  This is what tpg_mask_immersed_fields leaves.
 *
 * Arrays
 * - u, Gu at (Face, Center, Center) and v, Gv at (Center, Face, Center): padded parents of ONE geometry (Nx, Ny, Nz, Hx, Hy, Hz).
 * - w at (Center, Center, Face): a padded parent with Nz + 1 interior levels, Nz + 1 + 2 Hz planes, the same row pitch and plane.
 * - dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff: the grid's padded planes, halos built.  dz_f: Nz + 1 values.
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; ONE launch for both fields; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable into a
 * HIP graph.  Element offsets are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message:
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. a `scheme` other than TPG_MOMENTUM_ENSTROPHY_CONSERVING: TPG_ERR_UNSUPPORTED, the message names the value;
 *  3. null u, v or w, then null Gu or Gv, then a null metric plane or dz_f: TPG_ERR_INVALID_ARGUMENT;
 *  4. one of n_fc, n_cf without the other: TPG_ERR_INVALID_ARGUMENT;
 *  5. a pointer off its element alignment, a count plane off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  6. Gu or Gv overlapping u, v, w (whose parent is one level longer) or each other: TPG_ERR_INVALID_ARGUMENT;
 *  7. Hx < 1, Hy < 1 or Hz < 1: TPG_ERR_UNSUPPORTED;
 *  8. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (2, 1, 1) at halo (1, 1, 1) -- one chunk, one row, one level -- and up past 2^31
 * elements a parent (8640 x 4320 x 64 at halo 4, with n_fc, n_cf); a latitude band down to Hy rows gives the rows of the global call
 * (tests/test_gpu_tendency_edges.py). */
int tpg_momentum_advection_tendency(const void *u, const void *v, const void *w, void *Gu, void *Gv,
                                    const void *dx_fc, const void *dy_fc, const void *az_fc, const void *dx_cf, const void *dy_cf,
                                    const void *az_cf, const void *az_cc, const void *az_ff, const void *dz_f, const int32_t *n_fc,
                                    const int32_t *n_cf, double mask_value, int scheme, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                                    int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_MOMENTUM_H */
