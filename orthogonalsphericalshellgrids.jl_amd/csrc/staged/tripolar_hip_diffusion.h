/*
 * tripolar_hip_diffusion.h -- C ABI of libtripolar_hip_diffusion.so: the explicit diffusive tendency of a hydrostatic model with its top
 * and bottom boundary fluxes, on the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose
 * conventions hold here word for word: extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` =
 * TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a
 * HIP graph, no environment variable read.
 *
 * A library of its own, STAGED beside the table of the operator libraries (csrc/staged/, its own Makefile): the table's size, its headers,
 * its version scripts and the export list of every library in it are pinned, so this one enters the table in a change of its own.  The
 * libraries share no state: tpg_diffusion_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on
 * this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_DIFFUSION_H
#define TRIPOLAR_HIP_DIFFUSION_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_diffusion_last_error(void);

/* bits of `terms` of tpg_diffusive_tendency: the interior groups of the call.  Every other bit is refused with TPG_ERR_UNSUPPORTED. */
#define TPG_DIFFUSION_HORIZONTAL 1 /* the horizontal fluxes Fx, Fy with the number kappa_h; fields at (Center, Center) only */
#define TPG_DIFFUSION_VERTICAL 2   /* the vertical flux Fz at the faces k0+1..Nz with kappa_z */

/* `mode` of tpg_diffusive_tendency.  Every other value is refused with TPG_ERR_UNSUPPORTED, the message names it. */
#define TPG_DIFFUSION_ADD 0   /* G = G_old + D: after the advection and hydrostatic calls, before AB2 */
#define TPG_DIFFUSION_WRITE 1 /* G = D */

/* `kappa_z_form` of tpg_diffusive_tendency: what TPG_KAPPA_* mean in tripolar_hip_vertical_diffusion.h.  Every other value is refused
 * with TPG_ERR_UNSUPPORTED, the message names it. */
#define TPG_DIFFUSION_KAPPA_CONSTANT 0 /* `kappa_z` is NULL: T(kappa_z_value) on every face */
#define TPG_DIFFUSION_KAPPA_PROFILE 1  /* `kappa_z`: Nz + 1 device values at the faces 1..Nz+1 */
#define TPG_DIFFUSION_KAPPA_FIELD 2    /* `kappa_z`: a padded parent at (the fields' horizontal location, Face): face k at plane Hz + k - 1 */

/* ---- the explicit diffusive tendency with the top and bottom boundary fluxes --------------------------------------------------------------
 * ONE CALL IS UP TO TPG_MAX_FIELDS FIELDS AT ONE HORIZONTAL LOCATION, Center in z: c[q] and G[q] are padded parents of one geometry, and
 * the fields share every metric, the diffusivities, the count plane and the bottom height.  top_flux / bottom_flux: NULL, or a table of
 * `nfields` entries, each NULL or a padded 2-D plane (Ny+2Hy) x (Nx+2Hx) of `ft` of which only the interior is read.
 * [recalled: Oceananigans' diffusive_flux_x/y/z, div_dot_q at (Center, Center, Center), apply_z_bcs!, conditional_flux with
 * immersed_peripheral_node; parity unpinned, like every operator here]
 *
 * THE RULE, for every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with no
 * contraction.  Every operation is one correctly rounded IEEE operation.  F is the down-gradient transport kappa A dc, so no leading minus
 * appears.
 *     d = dz_c[k],  V = az[i,j] * d
 *     k0 = 1 without `counts`; with them k0 = min(max(counts[j,i], 0), Nz) + 1
 *   The horizontal group, present iff terms & TPG_DIFFUSION_HORIZONTAL; kh = T(kappa_h):
 *     Fx[i,j,k] = closed_x(i,j,k) ? T(0) : (kh * (dy_fc[i,j] * d)) * ((c[i,j,k] - c[i-1,j,k]) / dx_fc[i,j])      i = 1..Nx+1
 *     Fy[i,j,k] = closed_y(i,j,k) ? T(0) : (kh * (dx_cf[i,j] * d)) * ((c[i,j,k] - c[i,j-1,k]) / dy_cf[i,j])      j = 1..Ny+1
 *     Hsum = (Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])
 *   (dy_fc * d) and (dx_cf * d) are the Mx, My factors of tpg_tracer_advection_tendency, the same bits.
 *   The vertical group, present iff terms & TPG_DIFFUSION_VERTICAL, or top_flux != NULL, or bottom_flux != NULL -- a property of the call,
 *   not of a field or a level.  Face k lies between the cells k-1 and k; Jt, Jb are the field's planes:
 *     Fz[k]    = (kz[k] * az[i,j]) * ((c[k] - c[k-1]) / dz_f[k])   k = k0+1..Nz with TPG_DIFFUSION_VERTICAL, else T(0)
 *     Fz[k0]   = bottom_flux[q] ? -(az[i,j] * Jb[i,j]) : T(0)
 *     Fz[Nz+1] = top_flux[q]    ? -(az[i,j] * Jt[i,j]) : T(0)
 *     Vsum = Fz[k+1] - Fz[k]
 *   The result:
 *     S = Hsum, Vsum, or Hsum + Vsum: left to right over the groups that are present; an absent group is omitted, not added as a zero
 *     D = (T(1) / V) * S
 *     TPG_DIFFUSION_WRITE: G = D.  TPG_DIFFUSION_ADD: G = G_old + D.
 *     With `counts` the cells k < k0 of every G[q] receive T(mask_value), in both modes.
 * - Fluxes formed once.  Fx[i+1] of a column is Fx[i] of the next, Fy[j+1] of a row is Fy[j] of the next, Fz[k+1] of a level is Fz[k] of
 *   the next.  Recomputing one at a chunk edge gives the same bits.  Leading minus signs are sign flips.  V = 0 divides by it.
 * - Boundary fluxes.  A positive value is a flux in +z (Oceananigans' convention): a positive top flux removes the quantity, a positive
 *   bottom flux adds it.  The bottom flux enters the column's lowest wet cell k0; without `counts` that is k = 1, Oceananigans' rule; with
 *   `counts` it stands in for an immersed bottom flux condition [recalled].  With Nz = 1 both boundary faces sit on the one cell; in a
 *   column with one wet cell (k0 = Nz) likewise.  A column with k0 > Nz is all mask.
 * - Closed horizontal faces, with `bottom_height` (h: a padded 2-D plane of `ft`, halos filled, and z_centers, Nz values of `ft`: exactly
 *   the inputs of tpg_immersed_column_counts).  Cell (i,j,k) is inactive iff z_centers[k] <= h[i,j], compared in T, or j < 1 with
 *   south_is_wall.  closed_x(i,j,k) = inactive(i-1,j,k) || inactive(i,j,k); closed_y(i,j,k) = inactive(i,j-1,k) || inactive(i,j,k).  A NaN
 *   h compares false: the cell counts as active.  h is read one cell west, east, south and north of every interior column: row Ny + 1 is
 *   what the zipper fill left there, the columns 0 and Nx + 1 are the periodic ones; the kernel contains NO fold index map, so a latitude
 *   band is right whenever its seam halos are filled.  On one h, closed_x <=> k <= n_fc[i,j] and closed_y <=> k <= n_cf[i,j] wherever those
 *   dense planes of tpg_immersed_column_counts have an entry.  Without `bottom_height` no face is closed (and south_is_wall is not
 *   looked at): the project's older convention, the underlying grid's operator with the nodes under the bottom masked.
 * - Cells read.  With TPG_DIFFUSION_HORIZONTAL: c one cell west, east, south and north of the interior at the levels 1..Nz -- no corner
 *   cell, no z-halo plane -- so Hx >= 1 and Hy >= 1; the same cells of h; dy_fc, dx_fc at i = 1..Nx+1 and dx_cf, dy_cf at j = 1..Ny+1 of
 *   the interior rows and columns.  Without it: the node's own column only, every halo width the geometry check admits is accepted, no
 *   dx_* / dy_* plane is read (the pointers may be NULL) and `bottom_height` is not read.  az: the interior, the area plane at the fields'
 *   OWN location -- the same entry point serves u with az_fc (wind stress, explicit vertical viscosity) and v with az_cf.  Of kappa_z the
 *   faces 2..Nz are loaded and only the faces k0+1..Nz enter the result, as in tpg_vertical_implicit_diffusion: the faces 1 and Nz + 1 and
 *   every halo cell of a FIELD kappa are never read; of dz_f the same.  G is read only with TPG_DIFFUSION_ADD, its interior only.  Only
 *   interior cells of G are written.
 * - Diffusivities.  kappa_h is a number.  kappa_z takes the three forms, which give the same bits on equal values.
 * - The fields of a call go to the device in groups of 4, 2 and 1 per work item (of 2 and 1 with TPG_DIFFUSION_HORIZONTAL), one launch per
 *   group size; the bits are identical however they are grouped, and whether they are computed together or one by one.
 *
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; no atomics, no LDS, nothing allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element
 * offsets are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message:
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. nfields < 1 or nfields > TPG_MAX_FIELDS; a null table c or G; then a null entry c[q], G[q], the message names q:
 *     TPG_ERR_INVALID_ARGUMENT;
 *  3. `terms` with a bit other than the two above: TPG_ERR_UNSUPPORTED; a call in which no group is present (terms = 0 and both flux
 *     tables NULL): TPG_ERR_INVALID_ARGUMENT;
 *  4. a `mode` other than the two above, then a `kappa_z_form` other than the three above: TPG_ERR_UNSUPPORTED, the message names the value;
 *  5. null combinations, TPG_ERR_INVALID_ARGUMENT, in this order: `kappa_z` given with TPG_DIFFUSION_KAPPA_CONSTANT; `kappa_z` missing with
 *     TPG_DIFFUSION_KAPPA_PROFILE or TPG_DIFFUSION_KAPPA_FIELD; a null dz_c or az; a null dz_f with TPG_DIFFUSION_VERTICAL; a null dx_fc,
 *     dy_fc, dx_cf or dy_cf with TPG_DIFFUSION_HORIZONTAL; `bottom_height` without `z_centers`;
 *  6. with TPG_DIFFUSION_HORIZONTAL a kappa_h, or with TPG_DIFFUSION_VERTICAL and TPG_DIFFUSION_KAPPA_CONSTANT a kappa_z_value, that is not
 *     finite: TPG_ERR_INVALID_ARGUMENT;
 *  7. a pointer off its element alignment (a field, a G, a flux plane, then the shared arrays), `counts` off int32 alignment:
 *     TPG_ERR_INVALID_ARGUMENT;
 *  8. overlaps, TPG_ERR_INVALID_ARGUMENT: any G[q] with any c[r] (neighbours are read: this is not an in-place call), with a G[r], with a
 *     TPG_DIFFUSION_KAPPA_FIELD kappa_z, with a flux plane or with `bottom_height`;
 *  9. TPG_DIFFUSION_HORIZONTAL with Hx < 1 or Hy < 1: TPG_ERR_UNSUPPORTED, the message gives the stencil;
 * 10. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.  The plane check of 1. subsumes it today (a plane below 2^31 cells has fewer
 *     than 2^30 work items): no geometry reaches this message, it guards a change of either bound.
 * Everything else is served, down to (Nx, Ny, Nz) = (2, 1, 1) at halo (1, 1, 1). */
int tpg_diffusive_tendency(const void *const *c, void *const *G, int nfields, int terms, int mode, double kappa_h, const void *kappa_z,
                           double kappa_z_value, int kappa_z_form, const void *const *top_flux, const void *const *bottom_flux,
                           const void *dx_fc, const void *dy_fc, const void *dx_cf, const void *dy_cf, const void *az, const void *dz_c,
                           const void *dz_f, const int32_t *counts, double mask_value, const void *bottom_height, const void *z_centers,
                           int south_is_wall, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_DIFFUSION_H */
