/*
 * tripolar_hip_advection.h -- C ABI of libtripolar_hip_advection.so: the flux-form advection tendency of the tracers on the fields of a
 * TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word:
 * extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns
 * TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, the seventh, as the other operator libraries are: the export lists of the other six are pinned.  The libraries
 * share no state: tpg_advection_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on this
 * thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_ADVECTION_H
#define TRIPOLAR_HIP_ADVECTION_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_advection_last_error(void);

/* `scheme` of tpg_tracer_advection_tendency: the reconstruction of the tracer at the cell faces.  Centered, second order, is the only one
 * built; every other value is refused with TPG_ERR_UNSUPPORTED (upwind and WENO come later without an ABI change). */
#define TPG_ADVECTION_CENTERED2 0

/* ---- the tracer tendency a hydrostatic model's AB2 step consumes ------------------------------------------------------------------------
 * With `buoyancy = nothing`, no closure and no forcing, the tendency of a tracer is minus the divergence of its advective flux.  The result
 * is the `Gn` of tpg_ab2_step_fields (include/tripolar_hip_timestep.h); `w` is what tpg_w_from_continuity (include/tripolar_hip_continuity.h)
 * writes.
 * [recalled: Oceananigans' div_Uc with Centered(order = 2) in all three directions, _advective_tracer_flux_x/y/z, and
 * hydrostatic_free_surface_tracer_tendency with no diffusion and no forcing; parity unpinned, like every operator here]
 *
 * The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with
 * no contraction.  Every operation is one correctly rounded IEEE operation.
 *     d = dz_c[k]
 *     Mx[i,j,k] = (dy_fc[i,j] * d) * u[i,j,k]           i = 1..Nx+1     (the continuity's fe / fw, the same bits)
 *     My[i,j,k] = (dx_cf[i,j] * d) * v[i,j,k]           j = 1..Ny+1
 *     Mz[i,j,k] =  az_cc[i,j]      * w[i,j,k]           k = 1..Nz+1     (w has Nz+1 levels)
 *     Fx[i,j,k] = Mx[i,j,k] * (T(0.5) * (c[i-1,j,k] + c[i,j,k]))
 *     Fy[i,j,k] = My[i,j,k] * (T(0.5) * (c[i,j-1,k] + c[i,j,k]))
 *     Fz[i,j,k] = Mz[i,j,k] * (T(0.5) * (c[i,j,k-1] + c[i,j,k]))
 *     V = az_cc[i,j] * d
 *     G[i,j,k] = -((T(1) / V) * (((Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])) + (Fz[i,j,k+1] - Fz[i,j,k])))
 * - Shared fluxes.  Each flux is formed once: Fx[i+1] of a column is Fx[i] of the next, Fz[k+1] of a level is Fz[k] of the next.
 *   Recomputing one at a tile edge gives the same bits.
 * - Negation.  The leading minus is a sign flip.
 * - Zero volume.  V = 0 divides by it, as the rule says.
 * - Cells read.  c[0..Nx+1, j, k], c[i, 0..Ny+1, k] and c[i, j, 0..Nz+1]: a plus-shaped stencil, so no corner halo cell.
 *   u[1..Nx+1, j, k], v[i, 1..Ny+1, k], w[i, j, 1..Nz+1].  The same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.
 * - Halos.  Hx, Hy, Hz >= 1.  The caller has filled every halo of c, u and v.  w's interior is complete: w[1] and w[Nz+1] are interior
 *   faces of a (Center, Center, Face) field.
 * - Written.  Only interior cells of G.
 * - Mask.  With a (Center, Center) count plane n_cc (Ny x Nx int32, tpg_immersed_column_counts), the nodes k <= min(max(n, 0), Nz) of G
 *   hold T(mask_value) instead; everything is computed unmasked.  This is what tpg_mask_immersed_fields leaves on a Center field.
 * - Several tracers.  c[q] with G[q], q < nfields <= TPG_MAX_FIELDS, share one call.  Mx, My, Mz do not depend on the tracer:
 *   the results are bit-identical whether tracers are computed together or one by one.
 *
 * Arrays
 * - c[q], G[q], u at (Face, Center, Center) and v at (Center, Face, Center): padded parents of ONE geometry (Nx, Ny, Nz, Hx, Hy, Hz).
 * - w at (Center, Center, Face): a padded parent with Nz + 1 interior levels, Nz + 1 + 2 Hz planes, the same row pitch and plane.
 * - dy_fc, dx_cf, az_cc: the grid's padded planes, halos built.  dz_c: Nz values in the field type.
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element offsets
 * are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message:
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. a `scheme` other than TPG_ADVECTION_CENTERED2: TPG_ERR_UNSUPPORTED, the message names the value;
 *  3. nfields < 1 or nfields > TPG_MAX_FIELDS: TPG_ERR_INVALID_ARGUMENT;
 *  4. a null table c or G, then a null entry c[q] or G[q] (the message names q): TPG_ERR_INVALID_ARGUMENT;
 *  5. null u, v or w, then a null dy_fc, dx_cf, az_cc or dz_c: TPG_ERR_INVALID_ARGUMENT;
 *  6. a pointer off its element alignment (the message names it), n_cc off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  7. any G[q] overlapping any c[p], u, v, w (whose parent is one level longer) or another G: TPG_ERR_INVALID_ARGUMENT;
 *  8. Hx < 1, Hy < 1 or Hz < 1: TPG_ERR_UNSUPPORTED;
 *  9. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (2, 1, 1) at halo (1, 1, 1) -- one chunk, one row, one level -- and up past 2^31
 * elements a parent (8640 x 4320 x 64 at halo 4, with n_cc); a latitude band down to Hy rows gives the rows of the global call
 * (tests/test_gpu_tendency_edges.py). */
int tpg_tracer_advection_tendency(const void *const *c, void *const *G, int nfields, const void *u, const void *v, const void *w,
                                  const void *dy_fc, const void *dx_cf, const void *az_cc, const void *dz_c, const int32_t *n_cc,
                                  double mask_value, int scheme, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_ADVECTION_H */
