/*
 * tripolar_hip_weno.h -- C ABI of libtripolar_hip_weno.so: the flux-form advection tendency of the tracers with a fifth-order WENO
 * reconstruction in x and y on the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose
 * conventions hold here word for word: extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest,
 * `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable
 * into a HIP graph, no environment variable read.
 *
 * A library of its own, the ninth, as the other operator libraries are: the export lists of the other eight are pinned, and
 * tpg_tracer_advection_tendency (include/tripolar_hip_advection.h) keeps refusing every `scheme` but the centred one.  The libraries share
 * no state: tpg_weno_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on this thread; status
 * codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_WENO_H
#define TRIPOLAR_HIP_WENO_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_weno_last_error(void);

/* ---- the tracer tendency of the reference's drivers ---------------------------------------------------------------------------------------
 * examples/bickley_jet.jl builds FluxFormAdvection(WENO(; order = 5), WENO(; order = 5), Centered()): the tracer at an x- or y-face is
 * the fifth-order WENO reconstruction biased against the flow, at a z-face the centred mean.  The result is the `Gn` of
 * tpg_ab2_step_fields (include/tripolar_hip_timestep.h), as tpg_tracer_advection_tendency's is.
 * [recalled: Oceananigans' FluxFormAdvection(WENO(order = 5), WENO(order = 5), Centered()), uniform-grid coefficients, Jiang-Shu smoothness
 * indicators, WENO-Z weights, eps = 1e-8; parity unpinned, like every operator here]
 *
 * The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with
 * no contraction.  Every operation is one correctly rounded IEEE operation.  Mx, My, Mz, V, Fz and the last line are those of
 * tpg_tracer_advection_tendency, the same bits.
 *     K(n, d) = T(n) / T(d)                      a constant of the type;  eps = T(1e-8)
 *     S(a, b, c) = (a - T(2) * b) + c
 *
 *     R(q0, q1, q2, q3, q4):                     the face value; q2 is the upwind cell, q3 the downwind one
 *         p2 = (K(1,3) * q0 - K(7,6) * q1) + K(11,6) * q2
 *         p1 = (K(5,6) * q2 - K(1,6) * q1) + K(1,3)  * q3
 *         p0 = (K(1,3) * q2 + K(5,6) * q3) - K(1,6)  * q4
 *         s2 = S(q0,q1,q2);  d2 = (q0 - T(4) * q1) + T(3) * q2;          b2 = K(13,12) * (s2 * s2) + T(0.25) * (d2 * d2)
 *         s1 = S(q1,q2,q3);  d1 = q1 - q3;                                b1 = K(13,12) * (s1 * s1) + T(0.25) * (d1 * d1)
 *         s0 = S(q2,q3,q4);  d0 = (T(3) * q2 - T(4) * q3) + q4;           b0 = K(13,12) * (s0 * s0) + T(0.25) * (d0 * d0)
 *         tau = |b0 - b2|                                                 (a sign clear)
 *         r0 = tau / (b0 + eps);   r1 = tau / (b1 + eps);   r2 = tau / (b2 + eps)
 *         a0 = K(3,10) * (T(1) + r0 * r0);   a1 = K(3,5) * (T(1) + r1 * r1);   a2 = K(1,10) * (T(1) + r2 * r2)
 *         R  = ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2)
 *
 *     d = dz_c[k]
 *     Mx[i,j,k] = (dy_fc[i,j] * d) * u[i,j,k]           i = 1..Nx+1
 *     My[i,j,k] = (dx_cf[i,j] * d) * v[i,j,k]           j = 1..Ny+1
 *     Mz[i,j,k] =  az_cc[i,j]      * w[i,j,k]           k = 1..Nz+1     (w has Nz+1 levels)
 *     Fx[i,j,k] = Mx[i,j,k] * ( Mx[i,j,k] >= 0 ? R(c[i-3], c[i-2], c[i-1], c[i],   c[i+1])
 *                                              : R(c[i+2], c[i+1], c[i],   c[i-1], c[i-2]) )          (all at j, k)
 *     Fy[i,j,k] = My[i,j,k] * ( My[i,j,k] >= 0 ? R(c[j-3], c[j-2], c[j-1], c[j],   c[j+1])
 *                                              : R(c[j+2], c[j+1], c[j],   c[j-1], c[j-2]) )          (all at i, k)
 *     Fz[i,j,k] = Mz[i,j,k] * (T(0.5) * (c[i,j,k-1] + c[i,j,k]))
 *     V = az_cc[i,j] * d
 *     G[i,j,k] = -((T(1) / V) * (((Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])) + (Fz[i,j,k+1] - Fz[i,j,k])))
 * - One evaluation of R per face.  The right-biased value is R of the mirrored cells: five inputs are selected, R is evaluated once.
 * - The test `>= 0`.  It is true for -0 and false for NaN.
 * - Shared fluxes.  Each flux is formed once; recomputing one at a tile edge gives the same bits.
 * - Negation.  The leading minus is a sign flip.  Zero volume: V = 0 divides by it, as the rule says.
 * - Cells read.  c[-2..Nx+3, j, k], c[i, -2..Ny+3, k] and c[i, j, 0..Nz+1]: a plus-shaped stencil, so no corner halo cell.
 *   u[1..Nx+1, j, k], v[i, 1..Ny+1, k], w[i, j, 1..Nz+1].  The same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.
 * - Halos.  Hx >= 3, Hy >= 3, Hz >= 1.  The caller has filled every halo of c, u and v: the rows Ny+1..Ny+3 are the Zipper's, the rows
 *   -2..0 what the caller's south condition left there.  w's interior is complete.
 * - Written.  Only interior cells of G.
 * - Mask.  With a (Center, Center) count plane n_cc (Ny x Nx int32, tpg_immersed_column_counts), the nodes k <= min(max(n, 0), Nz) of G
 *   hold T(mask_value) instead; everything is computed unmasked.  This is what tpg_mask_immersed_fields leaves on a Center field.
 * - Several tracers.  c[q] with G[q], q < nfields <= TPG_MAX_FIELDS, share one call.  Mx, My, Mz do not depend on the tracer:
 *   the results are bit-identical however the tracers are grouped.
 * - Stays out.  Oceananigans' drop of the reconstruction order beside the south wall and beside immersed nodes (in both drivers every
 *   row south of -78 degrees and both pole boxes are under the mask, so the rows this touches are masked in the workloads here);
 *   stretched-grid coefficients; other orders; latitude bands; the Julia hooks (the momentum half: include/tripolar_hip_weno_momentum.h;
 *   WENO in z: include/tripolar_hip_weno_xyz.h, a call of its own).
 *
 * Arrays
 * - c[q], G[q], u at (Face, Center, Center) and v at (Center, Face, Center): padded parents of ONE geometry (Nx, Ny, Nz, Hx, Hy, Hz).
 * - w at (Center, Center, Face): a padded parent with Nz + 1 interior levels, Nz + 1 + 2 Hz planes, the same row pitch and plane.
 * - dy_fc, dx_cf, az_cc: the grid's padded planes, halos built.  dz_c: Nz values in the field type.
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element offsets
 * are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message (those of tpg_tracer_advection_tendency minus its scheme item):
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. nfields < 1 or nfields > TPG_MAX_FIELDS: TPG_ERR_INVALID_ARGUMENT;
 *  3. a null table c or G, then a null entry c[q] or G[q] (the message names q): TPG_ERR_INVALID_ARGUMENT;
 *  4. null u, v or w, then a null dy_fc, dx_cf, az_cc or dz_c: TPG_ERR_INVALID_ARGUMENT;
 *  5. a pointer off its element alignment (the message names it), n_cc off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  6. any G[q] overlapping any c[p], u, v, w (whose parent is one level longer) or another G: TPG_ERR_INVALID_ARGUMENT;
 *  7. Hx < 3, Hy < 3 or Hz < 1: TPG_ERR_UNSUPPORTED, the message names the stencil and the halo passed;
 *  8. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (4, 3, 1) at halo (3, 3, 1) -- Nx = Hx + 1, Ny = Hy: the arms end on the last halo
 * cell -- and (4, 4, 5) at halo (4, 4, 4), one chunk per row, and up past 2^31 elements a parent (8640 x 4320 x 64 at halo 4, with n_cc);
 * a latitude band down to Hy rows gives the rows of the global call (tests/test_gpu_tendency_edges.py). */
int tpg_weno_tracer_advection_tendency(const void *const *c, void *const *G, int nfields, const void *u, const void *v, const void *w,
                                       const void *dy_fc, const void *dx_cf, const void *az_cc, const void *dz_c, const int32_t *n_cc,
                                       double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_WENO_H */
