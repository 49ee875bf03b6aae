/*
 * tripolar_hip_weno_xyz.h -- C ABI of libtripolar_hip_weno_xyz.so: the flux-form advection tendency of the tracers with a fifth-order WENO
 * reconstruction in x, y AND z on the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose
 * conventions hold here word for word: extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest,
 * `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable
 * into a HIP graph, no environment variable read.
 *
 * A library of its own, the eleventh, as the other operator libraries are: the export lists of the other ten are pinned, and
 * tpg_weno_tracer_advection_tendency (include/tripolar_hip_weno.h: WENO in x and y, the centred mean in z) keeps its rule and its refusals.
 * The libraries share no state: tpg_weno_xyz_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY
 * on this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_WENO_XYZ_H
#define TRIPOLAR_HIP_WENO_XYZ_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_weno_xyz_last_error(void);

/* ---- the tracer tendency of `WENO()` -------------------------------------------------------------------------------------------------------
 * examples/distributed_bickley_jet.jl builds `tracer_advection = WENO()`: the tracer at an x-, y- AND z-face is the WENO reconstruction
 * biased against the flow, of order five away from the bottom and the surface and of a lower order beside them.  The result is the `Gn` of
 * tpg_ab2_step_fields (include/tripolar_hip_timestep.h), as tpg_weno_tracer_advection_tendency's is.
 * [recalled: Oceananigans' WENO() = FluxFormAdvection(WENO(order = 5) x3) on a z-Bounded grid; parity unpinned, like every operator here]
 *
 * The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with
 * no contraction.  Every operation is one correctly rounded IEEE operation.  Everything not named below is
 * include/tripolar_hip_weno.h's, with the same bits: K, eps, R (called R5 here), Mx, My, Mz, Fx, Fy, V, the last line, the mask, several
 * tracers.
 *
 *     R3(q0, q1, q2):                            the face value of order three; q1 is the upwind cell, q2 the downwind one
 *         p1 = T(1.5) * q1 - T(0.5) * q0
 *         p0 = T(0.5) * (q1 + q2)
 *         e1 = q1 - q0;  b1 = e1 * e1
 *         e0 = q2 - q1;  b0 = e0 * e0
 *         tau = |b0 - b1|                                                 (a sign clear)
 *         r0 = tau / (b0 + eps);   r1 = tau / (b1 + eps)
 *         a0 = K(2,3) * (T(1) + r0 * r0);   a1 = K(1,3) * (T(1) + r1 * r1)
 *         R3 = (a0 * p0 + a1 * p1) / (a0 + a1)
 *
 *     face f = 1..Nz+1 lies between the levels f-1 and f;   dist(f) = min(f - 1, Nz + 1 - f)
 *         dist = 0  (f = 1, f = Nz+1):  C = T(0.5) * (c[f-1] + c[f])                       the centred mean, as tripolar_hip_weno.h's Fz
 *         dist = 1:                     C = Mz >= 0 ? c[f-1] : c[f]
 *         dist = 2:                     C = Mz >= 0 ? R3(c[f-2], c[f-1], c[f])
 *                                                   : R3(c[f+1], c[f],   c[f-1])
 *         dist >= 3:                    C = Mz >= 0 ? R5(c[f-3], c[f-2], c[f-1], c[f],   c[f+1])
 *                                                   : R5(c[f+2], c[f+1], c[f],   c[f-1], c[f-2])
 *     Fz[i,j,f] = Mz[i,j,f] * C                                                             (all at i, j; Mz = Mz[i,j,f])
 *     G[i,j,k] = -((T(1) / V) * (((Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])) + (Fz[i,j,k+1] - Fz[i,j,k])))
 * - Order.  The order of a z-face depends on its distance from the nearer wall only, not on the flow's sign: Oceananigans' combined
 *   left-and-right bias test, as recalled.  Nz = 1: two centred faces, bit for bit tpg_weno_tracer_advection_tendency.  Nz = 2, 3: order 1
 *   appears.  Nz = 4: the first face of order 3.  Nz = 6: the first face of order 5.
 * - Selection.  `>= 0` is true for -0 and false for NaN.  The inputs are selected and the face value is evaluated once per face.
 * - Cells read in z.  A face with dist >= 1 reads levels 1..Nz only; faces 1 and Nz + 1 read the planes 0 and Nz + 1.  Nothing in the z-halo
 *   beyond those two planes is read at any Hz.  In x and y: tripolar_hip_weno.h's plus-shaped stencil, c[-2..Nx+3, j, k] and
 *   c[i, -2..Ny+3, k].  u[1..Nx+1, j, k], v[i, 1..Ny+1, k], w[i, j, 1..Nz+1]; the same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.
 * - Halos.  Hx >= 3, Hy >= 3, Hz >= 1, as tripolar_hip_weno.h's: no face of a reduced order reads a z-halo plane.
 * - Written.  Only interior cells of G.  Mask, several tracers, shared fluxes, negation, zero volume: tripolar_hip_weno.h's.
 * - Stays out.  Oceananigans' drop of the reconstruction order beside the south wall and beside immersed nodes, in all three directions now:
 *   faces above an immersed bottom take the full order on the masked cells below them.  Stretched-grid coefficients; other orders; latitude
 *   bands; the Julia hooks.
 *
 * Arrays: those of tpg_weno_tracer_advection_tendency, argument for argument.  Float32 and Float64, every pointer aligned to its element
 * type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned chunks otherwise; no atomics, nothing allocated,
 * asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element offsets are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message (those of tpg_weno_tracer_advection_tendency):
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. nfields < 1 or nfields > TPG_MAX_FIELDS: TPG_ERR_INVALID_ARGUMENT;
 *  3. a null table c or G, then a null entry c[q] or G[q] (the message names q): TPG_ERR_INVALID_ARGUMENT;
 *  4. null u, v or w, then a null dy_fc, dx_cf, az_cc or dz_c: TPG_ERR_INVALID_ARGUMENT;
 *  5. a pointer off its element alignment (the message names it), n_cc off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  6. any G[q] overlapping any c[p], u, v, w (whose parent is one level longer) or another G: TPG_ERR_INVALID_ARGUMENT;
 *  7. Hx < 3, Hy < 3 or Hz < 1: TPG_ERR_UNSUPPORTED, the message names the stencil
 *     "c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1]" and the halo passed;
 *  8. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (4, 3, 1) at halo (3, 3, 1) -- Nx = Hx + 1, Ny = Hy: the arms end on the last halo
 * cell -- and (4, 4, 1) at halo (4, 4, 4), one chunk per row, and up past 2^31 elements a parent (8640 x 4320 x 64 at halo 4, with n_cc);
 * a latitude band down to Hy rows gives the rows of the global call (tests/test_gpu_tendency_edges.py). */
int tpg_weno_xyz_tracer_advection_tendency(const void *const *c, void *const *G, int nfields, const void *u, const void *v, const void *w,
                                           const void *dy_fc, const void *dx_cf, const void *az_cc, const void *dz_c, const int32_t *n_cc,
                                           double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_WENO_XYZ_H */
