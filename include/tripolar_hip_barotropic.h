/*
 * tripolar_hip_barotropic.h -- C ABI of libtripolar_hip_barotropic.so: the barotropic mode of the 3-D velocities and the split-explicit velocity
 * correction on the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold
 * here word for word: extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64,
 * every call returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no
 * environment variable read.
 *
 * A library of its own, the fourth, as libtripolar_hip_operators.so and libtripolar_hip_continuity.so are: the export lists of the other three
 * are pinned.  The libraries share no state: tpg_barotropic_last_error() returns the thread-local message of the last failure of a call INTO
 * THIS LIBRARY on this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_BAROTROPIC_H
#define TRIPOLAR_HIP_BAROTROPIC_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_barotropic_last_error(void);

/* ---- the two ends of the split-explicit sub-cycle ----------------------------------------------------
 * A split-explicit free surface sub-cycles the 2-D fields eta, U, V between two passes over the 3-D velocities: the barotropic mode of the
 * predictor velocities before the sub-cycle, and the correction that makes the 3-D velocities carry the sub-cycled transport after it, before
 * w is diagnosed from continuity (tpg_w_from_continuity).
 * [recalled: Oceananigans' `compute_barotropic_mode!` and `barotropic_split_explicit_corrector!`; parity unpinned, like every operator here.]
 *
 * Arrays
 * - `u` at (Face, Center, Center) and `v` at (Center, Face, Center): padded parents of geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
 * - `U`, `V`, `Ubar`, `Vbar`: 2-D padded planes of `(Ny + 2 Hy2) x (Nx + 2 Hx)`: the same `Hx`, so the same row pitch as the 3-D fields, and
 *   THEIR OWN north / south halo `Hy2` >= 0 (the free surface's fields live on the extended-halo grid).
 * - `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]` in the field type, as in tpg_w_from_continuity.
 * Neither call has a stencil: every halo width >= 0 is accepted, no halo cell of any array is read, only interior cells are written.
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element offsets are
 * 64-bit.  Every check precedes any launch.
 *
 * tpg_barotropic_mode.  For every interior column `i = 1..Nx`, `j = 1..Ny`, in the field type, in exactly this order, no contraction, every
 * operation one correctly rounded IEEE operation:
 *     Ubar[i,j] = dz_c[1] * u[i,j,1]
 *     for k = 2..Nz:  Ubar[i,j] = Ubar[i,j] + dz_c[k] * u[i,j,k]
 * and Vbar from v likewise.  The mask is not an argument: levels under an immersed bottom ARE read (a model's u, v are masked there), as
 * tpg_w_from_continuity reads them.  ONE launch does both fields.  Either pair (u, Ubar) or (v, Vbar) may be NULL together, not both.
 * A work item owns one chunk of columns and walks ALL levels with the running sum in registers (level segments would re-associate the sum).
 * TPG_ERR_INVALID_ARGUMENT for every pointer NULL, a half-given pair, a null dz_c, an unknown ft, a pointer off its element alignment,
 * Ubar or Vbar overlapping u's or v's parent or each other, Hy2 < 0; TPG_ERR_UNSUPPORTED for more work items than 32 bits index.
 * u and v may be one array. */
int tpg_barotropic_mode(const void *u, const void *v, void *Ubar, void *Vbar, const void *dz_c,
                        int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int Hy2, int ft, void *stream);

/* tpg_barotropic_correction.  In place, for every interior node, in the field type:
 *     H = depth_of_count[min(n_fc[i,j], Nz)]        (n_fc NULL: depth_of_count[0])
 *     c = (U[i,j] - Ubar[i,j]) / H                  one subtraction, one division, formed once per column
 *     u[i,j,k] = u[i,j,k] + c      k = 1..Nz
 * and v likewise with V, Vbar, n_cf.  `H = 0` divides by it, as the rule says.
 * depth_of_count: `Nz + 1` values in the field type, depth_of_count[n] the depth of a column whose lowest n cells are immersed.
 * n_fc, n_cf: NULL, or the (Face, Center) / (Center, Face) count planes of tpg_immersed_column_counts, Ny x Nx int32.  Where a plane is given,
 * nodes k <= n get mask_value (converted once to the field type) instead: bit for bit what the call without the plane leaves after
 * tpg_mask_immersed_fields on u (plane fc, TPG_CENTER) and v (plane cf); a land column (H = +0, 0 / 0) is therefore wholly masked.
 * mask_value is not read when both planes are NULL.  Only the interior of U, V, Ubar, Vbar is read; no halo cell of u, v is read or written:
 * the caller's halo fill follows.  ONE launch does both fields.  A triple (u, U, Ubar) or (v, V, Vbar) may be NULL together, not both.
 * The checks of tpg_barotropic_mode, and: TPG_ERR_INVALID_ARGUMENT for a null depth_of_count, a count plane pointer off int32 alignment, a
 * 2-D plane overlapping u's or v's parent, u's parent overlapping v's (both are written). */
int tpg_barotropic_correction(void *u, void *v, const void *U, const void *V, const void *Ubar, const void *Vbar,
                              const void *depth_of_count, const int32_t *n_fc, const int32_t *n_cf, double mask_value,
                              int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int Hy2, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_BAROTROPIC_H */
