/*
 * tripolar_hip_free_surface.h -- C ABI of libtripolar_hip_free_surface.so: one forward-backward sub-step of a split-explicit free surface
 * (eta, U, V) on the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold
 * here word for word: extern "C", plain pointers, caller-owned DEVICE memory, padded arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every
 * call returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment
 * variable read.
 *
 * A library of its own, the fifth, as libtripolar_hip_operators.so, libtripolar_hip_continuity.so and libtripolar_hip_barotropic.so are: the
 * export lists of the other four are pinned.  The libraries share no state: tpg_free_surface_last_error() returns the thread-local message of
 * the last failure of a call INTO THIS LIBRARY on this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_FREE_SURFACE_H
#define TRIPOLAR_HIP_FREE_SURFACE_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_free_surface_last_error(void);

/* ---- the sub-step between the two ends of the split-explicit sub-cycle -------------------------------
 * tpg_barotropic_mode (tripolar_hip_barotropic.h) runs before the sub-cycle and tpg_barotropic_correction after it; this call is ONE of the
 * sub-steps between them, the caller's halo fill of (eta_out, U_out, V_out) follows each.
 * [recalled: Oceananigans' `_split_explicit_free_surface!` then `_split_explicit_barotropic_velocity!` on the new eta, ForwardBackwardScheme;
 * parity unpinned, like every operator here.]
 *
 * Arrays.  eta at (Center, Center), U, GU at (Face, Center), V, GV at (Center, Face), the averages eta_bar, U_bar, V_bar, and the five metric
 * planes dy_fc (Δyᶠᶜᵃ), dx_cf (Δxᶜᶠᵃ), az_cc (Azᶜᶜᵃ), dx_fc (Δxᶠᶜᵃ), dy_cf (Δyᶜᶠᵃ) are 2-D padded planes of ONE geometry
 * `(Ny + 2 Hy2) x (Nx + 2 Hx)`: the free surface's own extended-halo grid, as in tripolar_hip_barotropic.h.  depth_of_count: `Nz + 1` values
 * in the field type, as in tpg_barotropic_correction.  n_fc, n_cf: NULL, or the (Face, Center) / (Center, Face) count planes of
 * tpg_immersed_column_counts, Ny x Nx int32; a count is taken as min(max(n, 0), Nz).
 *
 * The rule.  In the field type, in exactly this order, no contraction, every operation one correctly rounded IEEE operation; dtau, g, weight
 * are converted once to the field type.
 *   Stage 1, for i = 1..Nx, j = 1..Ny:
 *     fe = dy_fc[i+1,j] * U[i+1,j]      fw = dy_fc[i,j] * U[i,j]
 *     fn = dx_cf[i,j+1] * V[i,j+1]      fs = dx_cf[i,j] * V[i,j]
 *     d  = ((fe - fw) + (fn - fs)) / az_cc[i,j]
 *     eta'[i,j] = eta[i,j] - dtau * d
 *   Stage 2, on eta', with eta'[0,j] = eta'[Nx,j] (the periodic wrap: recomputed, read from no halo):
 *     Hfc = depth_of_count[n_fc[i,j]]   (n_fc NULL: depth_of_count[0]);  gH = g * Hfc
 *     px  = (eta'[i,j] - eta'[i-1,j]) / dx_fc[i,j]
 *     U'[i,j] = U[i,j] + dtau * (GU[i,j] - gH * px)                                                       i = 1..Nx, j = 1..Ny
 *     V'[i,j] = V[i,j] + dtau * (GV[i,j] - (g * Hcf) * ((eta'[i,j] - eta'[i,j-1]) / dy_cf[i,j]))          j = 2..Ny
 *     V'[i,1] = V[i,1]                  (the south wall row is carried: the caller's Open fill owns it)
 *   Averaging (eta_bar, U_bar, V_bar NULL together, or all given), in place at the item's own cells:
 *     eta_bar = eta_bar + weight * eta',   U_bar = U_bar + weight * U',   V_bar = V_bar + weight * V'
 *
 * Cells.  Stage 1 reads the east halo column Nx+1 of U_in and dy_fc and the north halo row Ny+1 of V_in and dx_cf (the caller's fill put them
 * there): Hx >= 1 and Hy2 >= 1.  No other halo cell of any array is read; only interior cells are written.  No masking; H = 0 only drops the
 * pressure term; a zero metric divides, as the rule says.
 *
 * ONE launch per call.  A work item reads only the `_in` arrays and writes only eta_out, U_out, V_out (eta, U, V ping-pong: an in-place form
 * would race on the neighbour reads); the averages are the only arrays updated in place.  An item recomputes eta' at its west and south
 * neighbours: the same operations, hence the same bits as the owning item's.  16-B chunks where rows and pointers sit on the 16-B grid,
 * element-aligned chunks otherwise; no atomics, nothing allocated, no host wait, 64-bit element offsets, every check before any launch.
 *
 * TPG_ERR_INVALID_ARGUMENT for a NULL required pointer (everything but n_fc, n_cf and the averaging triple), a half-given averaging triple,
 * an unknown ft, a pointer off its element or int32 alignment, Hx < 1 or Hy2 < 1, eta_out, U_out, V_out or an average overlapping any other
 * array of the call (eta_in == eta_out included); TPG_ERR_UNSUPPORTED for Ny < 2 and for more work items than 32 bits index. */
int tpg_free_surface_substep(void *eta_out, void *U_out, void *V_out, const void *eta_in, const void *U_in, const void *V_in,
                             const void *GU, const void *GV, void *eta_bar, void *U_bar, void *V_bar,
                             const void *dy_fc, const void *dx_cf, const void *az_cc, const void *dx_fc, const void *dy_cf,
                             const void *depth_of_count, const int32_t *n_fc, const int32_t *n_cf,
                             double dtau, double g, double weight,
                             int Nx, int Ny, int Nz, int Hx, int Hy2, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_FREE_SURFACE_H */
