/*
 * tripolar_hip_mixing.h -- C ABI of libtripolar_hip_mixing.so: the vertical mixing diffusivities of a hydrostatic model -- convective
 * adjustment and Richardson-number-based mixing -- at the three locations the vertically implicit diffusion step wants them, on the fields
 * of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word:
 * extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns
 * TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, STAGED beside the table of the operator libraries (csrc/staged/, `make -C csrc/staged mixing`): the table's size,
 * its headers, its version scripts and the export list of every library in it are pinned, so this one enters the table in a change of its
 * own.  The libraries share no state: tpg_mixing_last_error() returns the thread-local message of the last failure of a call INTO THIS
 * LIBRARY on this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_MIXING_H
#define TRIPOLAR_HIP_MIXING_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_mixing_last_error(void);

/* ---- the vertical mixing diffusivities -------------------------------------------------------------------------------------------------------
 * Both calls share everything but the closure, which is a compile-time policy of ONE kernel template.
 * [recalled: Oceananigans' ConvectiveAdjustmentVerticalDiffusivity (compute_diffusivities!, is_stableᶜᶜᶠ) and RiBasedVerticalDiffusivity
 * (compute_ri_based_diffusivities!, Riᶜᶜᶠ, shear_squaredᶜᶜᶠ, PiecewiseLinearRiDependentTapering, the Cᵃᵛ time average), ℑxᶠᵃᵃ / ℑyᵃᶠᵃ of
 * the viscosity; parity unpinned, like every operator here]
 *
 * ARRAYS.  b, u, v: padded parents (Nz+2Hz) x (Ny+2Hy) x (Nx+2Hx) of `ft`, cell k at plane Hz + k - 1; b at (Center, Center, Center), u
 * at (Face, Center, Center), v at (Center, Face, Center).  kappa_c, nu_c, kappa_u, kappa_v and the two *_prev arrays: padded parents Face
 * in z, (Nz+1+2Hz) planes, face k at plane Hz + k - 1 -- what tpg_vertical_implicit_diffusion reads as a TPG_KAPPA_FIELD.  dz_f: Nz + 1
 * device values of `ft`, dz_f[k] the spacing between the centres k - 1 and k (the table of z_all_face_spacings).  n_cc, n_fc, n_cf: NULL
 * or int32 planes Ny x Nx without halos (tpg_immersed_column_counts).
 *
 * THE RULE, at the faces k = 2..Nz of every interior column i = 1..Nx, j = 1..Ny; face k lies between the cells k - 1 and k.  It is
 * evaluated in the field type T, in exactly this order, with no contraction; every operation is one correctly rounded IEEE operation and
 * divisions stay divisions.  half = T(0.5), one = T(1).
 *     N2(i,j,k) = (b[i,j,k] - b[i,j,k-1]) / dz_f[k]
 *   tpg_convective_adjustment_diffusivities:
 *     stable = (N2 >= 0)                       a NaN N2 compares false: NOT stable, the convective values
 *     kappa  = stable ? T(background_kappa) : T(convective_kappa)
 *     nu_c   = stable ? T(background_nu)    : T(convective_nu)
 *   tpg_ri_based_diffusivities, with du(i',j') = (u[i',j',k] - u[i',j',k-1]) / dz_f[k] and dv likewise:
 *     su = du(i,j)*du(i,j) + du(i+1,j)*du(i+1,j)
 *     sv = dv(i,j)*dv(i,j) + dv(i,j+1)*dv(i,j+1)
 *     S2 = half*su + half*sv
 *     Ri = (N2 == 0) ? T(0) : N2 / S2
 *     x  = (Ri - T(Ri0)) / T(Ri_delta);  y = (x > 0) ? x : T(0);  z = (y < one) ? y : one;  tau = one - z
 *     nu_i = T(nu0)*tau;  kappa_i = T(kappa0)*tau;  if (N2 < 0) kappa_i = kappa_i + T(kappa_ca)
 *     with the *_prev arrays:  nu_c  = (T(Cav)*nu_c_prev[i,j,k]    + nu_i)    / (one + T(Cav))
 *                              kappa = (T(Cav)*kappa_c_prev[i,j,k] + kappa_i) / (one + T(Cav))      (one + T(Cav) is formed once)
 *     without them:            nu_c = nu_i, kappa = kappa_i (Cav is not looked at beyond being finite)
 *   This is the piecewise-linear taper.  What the selects do with special values:
 *     N2 = +0 or -0          Ri = +0 whatever S2 is (0/0 is never formed); N2 < 0 is false, no kappa_ca
 *     S2 = 0, N2 > 0         Ri = +Inf, x = +Inf, y = +Inf, z = one, tau = 0
 *     S2 = 0, N2 < 0         Ri = -Inf, x = -Inf, y = 0, tau = one, and kappa_ca is added
 *     N2 or S2 NaN, Inf/Inf  Ri = NaN, x = NaN, (x > 0) is false: y = 0, tau = one -- full mixing; (NaN < 0) is false: no kappa_ca.  A NaN
 *                            in u or v alone therefore yields the finite values nu0, kappa0; a NaN in a *_prev array propagates
 *     x = -0                 y = +0
 *   The outputs, each optional through a NULL pointer:
 *     kappa_c[i,j,k] = kappa(i,j,k)                                (Center, Center, Face)
 *     nu_c[i,j,k]    = nu_c(i,j,k)                                 (Center, Center, Face)
 *     kappa_u[i,j,k] = half * (nu_c(i-1,j,k) + nu_c(i,j,k))        (Face, Center, Face)
 *     kappa_v[i,j,k] = half * (nu_c(i,j-1,k) + nu_c(i,j,k))        (Center, Face, Face)
 *   A work item forms nu_c of the column west of its chunk and of the row south of it by the SAME sequence of operations on values it loads
 *   itself: the bits are those of the neighbour's item.  One launch, no LDS, no second pass.
 * - Planes not evaluated.  The planes of the faces 1 and Nz + 1 of every output receive T(0) in the interior: closed faces, which the
 *   implicit solve never reads.  With Nz = 1 no face is evaluated.
 * - Masks.  With n_cc (for kappa_c and nu_c), n_fc (for kappa_u) or n_cf (for kappa_v), the faces k <= min(max(n[j,i], 0), Nz) + 1 of
 *   that output receive T(mask_value), the faces 1 and Nz + 1 included where they qualify.  A count plane whose output is NULL is not
 *   read.  Every face the three implicit calls then read at a location, k >= k0 + 1 with k0 the location's own lowest wet cell, has both
 *   of its contributing columns wet ((Face, Center) counts are the maximum of the two cells' counts): NO conditional interpolation is
 *   needed, and none is made.
 * - Cells read, per output, with own(i',j') = { b[i',j'] } for convective adjustment and
 *   own(i',j') = { b[i',j'], u[i',j'], u[i'+1,j'], v[i',j'], v[i',j'+1] } for the Ri rule, each at the levels 1..Nz:
 *     kappa_c: own(i,j), kappa_c_prev[i,j];   nu_c: own(i,j), nu_c_prev[i,j];
 *     kappa_u: own(i-1,j), own(i,j), nu_c_prev[i-1,j], nu_c_prev[i,j];   kappa_v: own(i,j-1), own(i,j), nu_c_prev[i,j-1], nu_c_prev[i,j].
 *   Over the interior that is one cell west, east, south and north of it -- and, for the Ri rule, the two corner cells u[Nx+1,0] (with
 *   kappa_v) and v[0,Ny+1] (with kappa_u) -- so the horizontal halos of b, u, v and of the *_prev arrays must be FILLED: row Ny + 1 is
 *   what the zipper fill left there, the columns 0 and Nx + 1 are the periodic ones.  The kernel contains NO fold index map, so a latitude
 *   band is right whenever its seam halos are filled.  No z-halo plane of an input is read; of the *_prev arrays and of dz_f only the
 *   faces 2..Nz.  Nothing else is read.  Hx >= 1 and Hy >= 1 are required whatever the outputs are.
 * - Cells written: the interior of the planes of the faces 1..Nz+1 of every output given.  No halo cell of an output is written.
 * - *_prev and the outputs may not overlap (neighbours are read while they are written): the caller ping-pongs them.
 *
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise (odd Hx, offset pointers, Float32 with Nx = 2 mod 4 as 8-B chunks); streaming stores; no atomics, no LDS, nothing
 * allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element offsets are 64-bit.  Every check precedes the
 * launch.
 *
 * Refusals, in this order, each with its own message:
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. null combinations, TPG_ERR_INVALID_ARGUMENT, in this order: a null b; (Ri) a null u or v; a null dz_f; no output at all; (Ri) one of
 *     kappa_c_prev and nu_c_prev without the other;
 *  3. the numbers, TPG_ERR_INVALID_ARGUMENT: a parameter that is not finite, named, in the order of the argument list; with a count plane
 *     a mask_value that is not finite; (Ri) Ri_delta <= 0; (Ri, with the *_prev arrays) one + T(Cav) == 0;
 *  4. a pointer off its element alignment (the inputs, then the outputs, then dz_f), a count plane off int32 alignment:
 *     TPG_ERR_INVALID_ARGUMENT;
 *  5. overlaps, TPG_ERR_INVALID_ARGUMENT: any output against any other array of the call, the message names both;
 *  6. Hx < 1 or Hy < 1: TPG_ERR_UNSUPPORTED, the message gives the stencil;
 *  7. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.  The plane check of 1. subsumes it today: no geometry reaches this message,
 *     it guards a change of either bound.
 * Everything else is served, down to (Nx, Ny, Nz) = (2, 1, 1) at halo (1, 1, 1). */
int tpg_convective_adjustment_diffusivities(const void *b, void *kappa_c, void *nu_c, void *kappa_u, void *kappa_v, double background_kappa,
                                            double convective_kappa, double background_nu, double convective_nu, const void *dz_f,
                                            const int32_t *n_cc, const int32_t *n_fc, const int32_t *n_cf, double mask_value, int Nx, int Ny,
                                            int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

int tpg_ri_based_diffusivities(const void *b, const void *u, const void *v, const void *kappa_c_prev, const void *nu_c_prev, void *kappa_c,
                               void *nu_c, void *kappa_u, void *kappa_v, double nu0, double kappa0, double kappa_ca, double Ri0,
                               double Ri_delta, double Cav, const void *dz_f, const int32_t *n_cc, const int32_t *n_fc, const int32_t *n_cf,
                               double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_MIXING_H */
