/*
 * tripolar_hip_hydrostatic.h -- C ABI of libtripolar_hip_hydrostatic.so: the Coriolis and the hydrostatic pressure-gradient tendencies of the
 * horizontal velocities, and the hydrostatic pressure anomaly itself, on the fields of a TripolarGrid for MI355X (gfx950), beside
 * libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word: extern "C", plain pointers, caller-owned DEVICE
 * memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a positive
 * hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, the fourteenth, as the other operator libraries are: the export lists of the other thirteen are pinned.  The
 * libraries share no state: tpg_hydrostatic_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on
 * this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_HYDROSTATIC_H
#define TRIPOLAR_HIP_HYDROSTATIC_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_hydrostatic_last_error(void);

/* `coriolis_scheme` of tpg_hydrostatic_tendencies.  Every other value is refused with TPG_ERR_UNSUPPORTED, the message names it
 * (Oceananigans' ActiveCellEnstrophyConserving is not built). */
#define TPG_CORIOLIS_ENSTROPHY_CONSERVING 0
#define TPG_CORIOLIS_ENERGY_CONSERVING 1

/* `mode` of tpg_hydrostatic_tendencies: accumulate into what Gu, Gv hold, or write. */
#define TPG_TENDENCY_ADD 0
#define TPG_TENDENCY_WRITE 1

/* ---- what a hydrostatic model with Coriolis and a buoyancy tracer adds to the velocity tendencies ------------------------------------------
 * With `coriolis = HydrostaticSphericalCoriolis()` and `buoyancy = BuoyancyTracer()` the tendency of u is -U.grad(u) - f x U - d/dx p, p the
 * hydrostatic pressure anomaly: the integral of b from the surface down.  The advection calls (include/tripolar_hip_momentum.h and the WENO
 * ones) leave -U.grad(u), -U.grad(v) in Gu, Gv; this call continues that left-to-right sum in place (TPG_TENDENCY_ADD), or writes the two
 * terms alone (TPG_TENDENCY_WRITE).  The results are the `Gu`, `Gv` of tpg_ab2_step_velocities (include/tripolar_hip_timestep.h).
 * [recalled: Oceananigans' update_hydrostatic_pressure!, the pressure gradient d/dx (Face, Center, Center) of pHY', and x_f_cross_U /
 * y_f_cross_U of HydrostaticSphericalCoriolis with the EnstrophyConserving and EnergyConserving schemes; parity unpinned, like every
 * operator here]
 *
 * THE RULE covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with no
 * contraction.  Every operation is one correctly rounded IEEE operation.
 *     PH[i,j,Nz] = -((T(0.5) * (b[i,j,Nz] + b[i,j,Nz+1])) * dz_f[Nz+1])
 *     PH[i,j,k]  = PH[i,j,k+1] - ((T(0.5) * (b[i,j,k] + b[i,j,k+1])) * dz_f[k+1])        k = Nz-1 .. 1, in this order
 *     px = (PH[i,j,k] - PH[i-1,j,k]) / dx_fc[i,j]          py = (PH[i,j,k] - PH[i,j-1,k]) / dy_cf[i,j]
 *
 *     P[i,j,k] = dx_cf[i,j] * v[i,j,k]     Q[i,j,k] = dy_fc[i,j] * u[i,j,k]      (tpg_momentum_advection_tendency's P, Q)
 *   TPG_CORIOLIS_ENSTROPHY_CONSERVING:
 *     fb = T(0.5) * (f_ff[i,j] + f_ff[i,j+1]);  vh = T(0.5) * (T(0.5) * (P[i-1,j,k] + P[i-1,j+1,k]) + T(0.5) * (P[i,j,k] + P[i,j+1,k]))
 *     cu = (fb * vh) / dx_fc[i,j]
 *     fb = T(0.5) * (f_ff[i,j] + f_ff[i+1,j]);  uh = T(0.5) * (T(0.5) * (Q[i,j-1,k] + Q[i+1,j-1,k]) + T(0.5) * (Q[i,j,k] + Q[i+1,j,k]))
 *     cv = (fb * uh) / dy_cf[i,j]
 *   TPG_CORIOLIS_ENERGY_CONSERVING:
 *     VX[i,j,k] = T(0.5) * (P[i-1,j,k] + P[i,j,k]);   cu = (T(0.5) * (f_ff[i,j] * VX[i,j,k] + f_ff[i,j+1] * VX[i,j+1,k])) / dx_fc[i,j]
 *     UY[i,j,k] = T(0.5) * (Q[i,j-1,k] + Q[i,j,k]);   cv = (T(0.5) * (f_ff[i,j] * UY[i,j,k] + f_ff[i+1,j] * UY[i+1,j,k])) / dy_cf[i,j]
 *
 *   mode TPG_TENDENCY_ADD:    Gu = (Gu + cu) - px        Gv = (Gv - cv) - py
 *   mode TPG_TENDENCY_WRITE:  Gu =  cu - px              Gv = (-cv) - py
 * - Shared quantities.  Each of PH, P, Q, VX, UY has one definition: forming it once or again at a tile edge gives the same bits.
 * - Signs.  Leading minus signs are sign flips.  ADD onto a field of -0 gives WRITE's bits (-0 is the additive identity; +0 is not, at
 *   cu = -0).
 * - Zero divisors.  A zero divisor divides, as the rule says.  A model masks the nodes at the grid poles.
 * - Either term may be absent.  f_ff == NULL drops the Coriolis operation: u, v, dx_cf and dy_fc may then be NULL too.  b == NULL drops the
 *   pressure operation: dz_f may then be NULL too.  The dropped operation is omitted, not replaced by a zero:
 *       ADD:   Gu = Gu + cu, Gv = Gv - cv      or   Gu = Gu - px, Gv = Gv - py
 *       WRITE: Gu = cu,      Gv = -cv          or   Gu = -px,     Gv = -py
 * - p_out.  Nullable, at (Center, Center, Center), a padded parent of the same geometry.  It receives PH on the interior, unmasked.  With
 *   Gu and Gv both NULL, b and p_out are required and the call is update_hydrostatic_pressure! alone: f_ff, u, v, the metric planes, the
 *   count planes, coriolis_scheme's term and mode's are then not used.
 * - f_ff.  An INPUT plane at (Face, Face), padded like the metric planes: the kernel evaluates no sine, so its parity does not depend on
 *   how f was made.
 * - dz_f.  Nz + 1 values in the field type: the centre-to-centre spacing at faces 1..Nz+1 (the table of tpg_momentum_advection_tendency).
 *   The factor at the top face is the FULL spacing dz_f[Nz+1], as the recalled rule has it.
 * - Cells read, relative to the node, over the interior:
 *       array   for Gu                                       for Gv
 *       v       (-1,0), (-1,+1), (0,0), (0,+1)               not read
 *       u       not read                                     (0,-1), (+1,-1), (0,0), (+1,0)
 *       dx_cf   as v                                         not read
 *       dy_fc   not read                                     as u
 *       f_ff    (0,0), (0,+1)                                (0,0), (+1,0)
 *       b       (0,0), (-1,0) at every level k .. Nz+1       (0,0), (0,-1) at every level k .. Nz+1
 *       dx_fc   (0,0)                                        not read
 *       dy_cf   not read                                     (0,0)
 *   and Gu, Gv at the node itself in ADD mode; for p_out, b at (0,0) at every level k .. Nz+1.  The corner cells v[0, Ny+1] and u[Nx+1, 0]
 *   ARE read.  Plane 0 of b and its corner columns are never read.
 * - Halos.  Hx, Hy, Hz >= 1.  The caller has filled the horizontal halos of u, v and every halo of b; the no-flux top halo of b is what
 *   tpg_fill_bounded_halos leaves.
 * - Written.  Only interior cells of Gu, Gv and p_out.  A node of Gu, Gv is read and written by the same work item: in place is safe.
 * - Mask.  n_fc and n_cf, the (Face, Center) and (Center, Face) count planes (Ny x Nx int32, tpg_immersed_column_counts), are both given
 *   or both NULL.  With them, the nodes k <= min(max(n, 0), Nz) of Gu (by n_fc) and of Gv (by n_cf) hold T(mask_value) instead, in both
 *   modes; everything is computed unmasked, p_out is not masked.  This is what tpg_mask_immersed_fields leaves.
 *
 * Arrays
 * - u, Gu at (Face, Center, Center), v, Gv at (Center, Face, Center), b, p_out at (Center, Center, Center): padded parents of ONE geometry
 *   (Nx, Ny, Nz, Hx, Hy, Hz).
 * - f_ff, dx_fc, dy_fc, dx_cf, dy_cf: padded planes, halos built.  dz_f: Nz + 1 values.
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; ONE launch for everything; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable into a
 * HIP graph.  Element offsets are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message:
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. a `coriolis_scheme` other than the two above, then a `mode` other than the two above: TPG_ERR_UNSUPPORTED, the message names the value;
 *  3. neither f_ff nor b: TPG_ERR_INVALID_ARGUMENT;
 *  4. null combinations, TPG_ERR_INVALID_ARGUMENT: one of Gu, Gv without the other; Gu and Gv both NULL without b and p_out; p_out without
 *     b; with Gu and Gv, a null dx_fc or dy_cf; with Gu, Gv and f_ff, a null u, v, dx_cf or dy_fc; b without dz_f;
 *  5. one of n_fc, n_cf without the other: TPG_ERR_INVALID_ARGUMENT;
 *  6. a pointer off its element alignment, a count plane off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  7. Gu, Gv or p_out overlapping u, v, b or each other: TPG_ERR_INVALID_ARGUMENT;
 *  8. Hx < 1, Hy < 1 or Hz < 1: TPG_ERR_UNSUPPORTED;
 *  9. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (2, 1, 1) at halo (1, 1, 1); a latitude band with its halo rows filled gives the rows
 * of the global call. */
int tpg_hydrostatic_tendencies(const void *u, const void *v, const void *b, void *Gu, void *Gv, void *p_out,
                               const void *f_ff, const void *dx_fc, const void *dy_fc, const void *dx_cf, const void *dy_cf,
                               const void *dz_f, const int32_t *n_fc, const int32_t *n_cf, double mask_value,
                               int coriolis_scheme, int mode, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_HYDROSTATIC_H */
