/*
 * tripolar_hip_weno_vi.h -- C ABI of libtripolar_hip_weno_vi.so: the vector-invariant advection tendency of the horizontal velocities with
 * the WENO5-upwinded vorticity term, the upwinded vertical term and the upwinded kinetic-energy gradient on the fields of a TripolarGrid for
 * MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word: extern "C", plain
 * pointers, caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative
 * tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, the twelfth, as the other operator libraries are: the export lists of the other eleven are pinned, and
 * tpg_weno_momentum_advection_tendency (include/tripolar_hip_weno_momentum.h) keeps its rule and its refusals.  The libraries share no
 * state: tpg_weno_vi_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on this thread; status
 * codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_WENO_VI_H
#define TRIPOLAR_HIP_WENO_VI_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_weno_vi_last_error(void);

/* ---- the velocity tendencies with upwinding in every term ------------------------------------------------------------------------------------
 * The scheme is Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(), vertical_scheme =
 * WENO(order = 5), kinetic_energy_gradient_scheme = WENO(order = 5), divergence_scheme = WENO(order = 5), upwinding =
 * OnlySelfUpwinding(cross_scheme = WENO(order = 5))): the drivers' WENOVectorInvariant(vorticity_order = 5) but for the smoothness stencil of
 * the vorticity reconstruction (DefaultStencil here, VelocityStencil there).  The vorticity term is
 * tpg_weno_momentum_advection_tendency's; the vertical term is the flux form u * div_h + d/dz(W u) with the divergence upwinded against the
 * advected velocity itself and the z-flux reconstructed by WENO; the kinetic-energy gradient is upwinded the same way.  The results are the
 * `Gu`, `Gv` of tpg_ab2_step_velocities (include/tripolar_hip_timestep.h).
 * [recalled: Oceananigans' upwinded_divergence_flux_U / _V and bernoulli_head_U / _V for VectorInvariant with WENO schemes and
 * OnlySelfUpwinding: the self term reconstructed with FunctionStencil smoothness (the divergence measured on the whole divergence, the
 * kinetic-energy difference on the mean velocity), the cross term taken as the symmetric value of the WENO scheme (Centered of order 4);
 * vertical_advection_U / _V as the flux form with the z-face orders of a Bounded column; parity unpinned, like every operator here]
 *
 * THE RULE covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with
 * no contraction.  Every operation is one correctly rounded IEEE operation.  Z, P, Q, A, vh, uh are include/tripolar_hip_momentum.h's and
 * hu, hv include/tripolar_hip_weno_momentum.h's, bit for bit: the vorticity term is the built one, DefaultStencil smoothness included.
 *
 *   C4(a, b, c, d) = (T(7)/T(12)) * (b + c) - (T(1)/T(12)) * (a + d)
 *       the symmetric value of a WENO(order = 5) scheme, Centered of order 4, between b and c
 *   W5F(q0..q4; s0..s4) = R(q0..q4) of include/tripolar_hip_weno.h with one change: s2, s1, s0, d2, d1, d0 -- and so b2, b1, b0 -- are formed
 *       from s0..s4; p2, p1, p0 are formed from q0..q4.  The smoothness is measured on another function than the one reconstructed
 *       (Oceananigans' FunctionStencil).  W5F(q; q) is R(q), the same bits.
 *   ZF(x, M, f) = the z-face value C of include/tripolar_hip_weno_xyz.h at face f = 1..Nz+1 of the column x[.], with M in place of Mz: the
 *       centred mean at distance 0 from a wall, the upwind cell at distance 1, R3 at distance 2, R5 at distance 3 and more; `M >= 0`
 *       selects.
 *
 *   per level (i, j range over what the stencils below need; dz_c[k] is the thickness of level k)
 *     FX[i,j,k]  = Q[i,j,k] * dz_c[k]                 FY[i,j,k]  = P[i,j,k] * dz_c[k]
 *     DU[i,j,k]  = FX[i+1,j,k] - FX[i,j,k]            DV[i,j,k]  = FY[i,j+1,k] - FY[i,j,k]            DS = DU + DV
 *     HU         = T(0.5) * (u*u)                     HV         = T(0.5) * (v*v)
 *     DKU[i,j,k] = HU[i+1,j,k] - HU[i,j,k]            DKV[i,j,k] = HV[i,j+1,k] - HV[i,j,k]            (at centres)
 *     XKV[i,j,k] = HV[i,j,k] - HV[i-1,j,k]            XKU[i,j,k] = HU[i,j,k] - HU[i,j-1,k]            (at (Face, Face))
 *     SU[i,j,k]  = T(0.5) * (u[i,j,k] + u[i+1,j,k])   SV[i,j,k]  = T(0.5) * (v[i,j,k] + v[i,j+1,k])
 *
 *   u, with uu = u[i,j,k]:
 *     dvs = C4(DV[i-2,j], DV[i-1,j], DV[i,j], DV[i+1,j])
 *     dur = uu >= 0 ? W5F(DU[i-3..i+1, j]; DS[i-3..i+1, j])
 *                   : W5F(DU[i+2..i-2, j]; DS[i+2..i-2, j])
 *     Wu[i,j,f]  = C4(A[i-2,j,f], A[i-1,j,f], A[i,j,f], A[i+1,j,f])
 *     FZu[i,j,f] = Wu * ZF(u[i,j,.], Wu, f)                                                       f = 1..Nz+1
 *     vu  = (uu * (dvs + dur) + (FZu[i,j,k+1] - FZu[i,j,k])) / (az_fc[i,j] * dz_c[k])
 *     kus = C4(XKV[i,j-1], XKV[i,j], XKV[i,j+1], XKV[i,j+2])
 *     kur = uu >= 0 ? W5F(DKU[i-3..i+1, j]; SU[i-3..i+1, j])
 *                   : W5F(DKU[i+2..i-2, j]; SU[i+2..i-2, j])
 *     bu  = (kur + kus) / dx_fc[i,j]
 *     Gu[i,j,k] = -((hu + vu) + bu)
 *
 *   v, with vv = v[i,j,k], the mirror image:
 *     dus = C4(DU[i,j-2], DU[i,j-1], DU[i,j], DU[i,j+1])
 *     dvr = vv >= 0 ? W5F(DV[i, j-3..j+1]; DS[i, j-3..j+1])
 *                   : W5F(DV[i, j+2..j-2]; DS[i, j+2..j-2])
 *     Wv[i,j,f]  = C4(A[i,j-2,f], A[i,j-1,f], A[i,j,f], A[i,j+1,f])
 *     FZv[i,j,f] = Wv * ZF(v[i,j,.], Wv, f)
 *     vvert = (vv * (dus + dvr) + (FZv[i,j,k+1] - FZv[i,j,k])) / (az_cf[i,j] * dz_c[k])
 *     kvs = C4(XKU[i-1,j], XKU[i,j], XKU[i+1,j], XKU[i+2,j])
 *     kvr = vv >= 0 ? W5F(DKV[i, j-3..j+1]; SV[i, j-3..j+1])
 *                   : W5F(DKV[i, j+2..j-2]; SV[i, j+2..j-2])
 *     bv  = (kvr + kvs) / dy_cf[i,j]
 *     Gv[i,j,k] = -((hv + vvert) + bv)
 *
 * - Shared quantities.  Each of Z, P, Q, A, FX, FY, DU, DV, DS, HU, HV, DKU, DKV, XKU, XKV, SU, SV, Wu, Wv, FZu, FZv has one definition:
 *   forming it once, again at a chunk's edge or in another launch gives the same bits.
 * - Selection.  `>= 0` is true for -0 and false for NaN.  The ten inputs of a W5F are selected and it is evaluated once per node and term;
 *   ZF selects its inputs and evaluates its face value once per face.
 * - Signs, zero divisors.  Leading minus signs are sign flips.  A zero divisor divides: zero az_ff, az_fc, az_cf, dx_fc or dy_cf at the grid
 *   poles, or a zero dz_c, give Inf or NaN.  A model masks them.
 * - dz_c.  Nz values in the field type: the thickness of the levels 1..Nz.  There is no dz_f: the flux-form vertical term does not use it.
 * - Cells read, relative to the node, over the interior, at the node's level.  u at (-3..+3, 0), (-2..+3, -1), (0, -3..+3) and
 *   (1, -3..+2); v at (0, -3..+3), (-1, -2..+3), (-3..+3, 0) and (-3..+2, 1): the arms end three cells out in x and y, and corner halo
 *   cells ARE read (u[Nx+3, 0], v[0, Ny+3]).  w at the faces k, k+1 at (-2..+1, 0) and (0, -2..+1): two cells out.  In z, u and v at
 *   (0, 0) at the levels the two faces of the node read by the order table: within k-3..k+3 and within 0..Nz+1.  Metric planes: dx_fc at
 *   (0, -3..+3) and (-2..+3, -1..0); dy_cf at (-1..0, -2..+3) and (-3..+3, 0); az_ff at (0, -2..+3) and (-2..+3, 0); dy_fc at (-3..+3, 0)
 *   and (0..1, -3..+2); dx_cf at (0, -3..+3) and (-3..+2, 0..1); az_cc at (-2..+1, 0) and (0, -2..+1); az_fc and az_cf at (0, 0).
 * - Halos.  Hx >= 3, Hy >= 3, Hz >= 1, w's horizontal halos included.  No face of a reduced order reads a z-halo plane beyond 0 and
 *   Nz + 1: faces 1 and Nz + 1 read those two planes, every other face levels 1..Nz only.  The caller has filled every halo of u and v
 *   and the horizontal halos of w.  The rows Ny+1..Ny+3 are the Zipper's, the rows -2..0 what the south condition left there.
 * - Written.  Only interior cells of Gu and Gv.  The call may use them as its own scratch before the final values are stored.
 * - Non-finite values.  A non-finite Z[i,j] reaches what it reaches in include/tripolar_hip_weno_momentum.h: the six Gu nodes
 *   (i, j-3..j+2) and the six Gv nodes (i-3..i+2, j).  A non-finite DU[i,j] reaches the Gu nodes (i-2..i+3, j) -- through dur and, as DS,
 *   through its smoothness -- and the Gv nodes (i, j-2..j+3); a non-finite DV[i,j] the Gv nodes (i, j-2..j+3) and the Gu nodes
 *   (i-2..i+3, j).  A non-finite u[i,j,k] reaches every node that reads it: beside those of its Z, DU, DKU, SU and XKU, the levels
 *   k-3..k+3 of its own column through ZF, where a level's faces read it.  Each arrives as NaN wherever a smoothness indicator holds it.
 * - Mask.  As in include/tripolar_hip_momentum.h: with n_fc and n_cf, the nodes k <= min(max(n, 0), Nz) hold T(mask_value); everything is
 *   computed unmasked, and ZF above an immersed bottom takes the full order on the masked cells below.
 * - Stays out.  VelocityStencil smoothness of the vorticity reconstruction, which alone separates this from the drivers' scheme;
 *   Oceananigans' drop of the order beside the south wall and immersed nodes; stretched-grid coefficients; other orders.
 *
 * Arrays: those of tpg_weno_momentum_advection_tendency, argument for argument, with dz_c (Nz values) where dz_f stood.  Float32 and
 * Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned chunks
 * otherwise; no atomics, no LDS, nothing allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.  TWO launches on
 * `stream`: the first leaves hu, hv in Gu, Gv, the second reads them back at its own nodes and finishes -((hu + vu) + bu) -- the order of
 * the three additions is kept, so the bits are those of one evaluation.  Element offsets are 64-bit.  Every check precedes any launch.
 *
 * Refusals, in this order, each with its own message (tpg_weno_momentum_advection_tendency's, with dz_c where dz_f stood):
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. null u, v or w, then null Gu or Gv, then a null metric plane or dz_c: TPG_ERR_INVALID_ARGUMENT;
 *  3. one of n_fc, n_cf without the other: TPG_ERR_INVALID_ARGUMENT;
 *  4. a pointer off its element alignment, a count plane off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  5. Gu or Gv overlapping u, v, w (whose parent is one level longer) or each other: TPG_ERR_INVALID_ARGUMENT;
 *  6. Hx < 3, Hy < 3 or Hz < 1: TPG_ERR_UNSUPPORTED, the message names the stencil and the halo passed;
 *  7. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (4, 3, 1) at halo (3, 3, 1) -- Nx = Hx + 1, Ny = Hy: the arms end on the last halo
 * cell -- and (4, 4, 5) at halo (4, 4, 4), and up past 2^31 elements a parent (8640 x 4320 x 64 at halo 4, with n_fc, n_cf); a latitude
 * band down to Hy rows gives the rows of the global call. */
int tpg_weno_vi_momentum_advection_tendency(const void *u, const void *v, const void *w, void *Gu, void *Gv,
                                            const void *dx_fc, const void *dy_fc, const void *az_fc, const void *dx_cf, const void *dy_cf,
                                            const void *az_cf, const void *az_cc, const void *az_ff, const void *dz_c, const int32_t *n_fc,
                                            const int32_t *n_cf, double mask_value, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                                            int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_WENO_VI_H */
