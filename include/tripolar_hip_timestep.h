/*
 * tripolar_hip_timestep.h -- C ABI of libtripolar_hip_timestep.so: the quasi-Adams-Bashforth-2 step of the velocities and the tracers and the
 * barotropic forcing of a split-explicit free surface on the fields of a TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so
 * (include/tripolar_hip.h), whose conventions hold here word for word: extern "C", plain pointers, caller-owned DEVICE memory, padded parent
 * arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on
 * `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, the sixth, as the other operator libraries are: the export lists of the other five are pinned.  The libraries share
 * no state: tpg_timestep_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY on this thread; status
 * codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_TIMESTEP_H
#define TRIPOLAR_HIP_TIMESTEP_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_timestep_last_error(void);

/* flag bits of both calls */
#define TPG_AB2_EULER 1          /* a first step: g = c1 * Gn, the previous tendency is NOT read */
#define TPG_AB2_STORE_PREVIOUS 2 /* Gm[i,j,k] = Gn[i,j,k] after the step (store_tendencies!) */

/* ---- the head of the split-explicit step ----------------------------------------------------------------
 * A hydrostatic model turns the tendencies of this step, Gn, and of the previous one, Gm, into new velocities and tracers, and -- with a
 * split-explicit free surface -- into the forcing GU, GV its sub-cycle integrates (tpg_free_surface_substep), before the barotropic mode
 * (tpg_barotropic_mode), the sub-cycle, the correction (tpg_barotropic_correction) and w (tpg_w_from_continuity).
 * [recalled: Oceananigans' QuasiAdamsBashforth2 `ab2_step_velocities!`, `ab2_step_tracers!`, `store_tendencies!` and, for a split-explicit
 * free surface, `_compute_integrated_ab2_tendencies!`; parity unpinned, like every operator here.]
 *
 * The rule, for every interior node, in the field type T, in exactly this order, no contraction, every operation one correctly rounded IEEE
 * operation; `dt` and `chi` arrive as doubles and are converted to T once:
 *     c1 = T(1.5) + chi_T          c2 = T(0.5) + chi_T          one addition each, formed once per call
 *     g  = c1 * Gn[i,j,k] - c2 * Gm[i,j,k]                      two products, one subtraction
 *          with TPG_AB2_EULER:  g = c1 * Gn[i,j,k]              Gm is NOT read: a first step's previous tendency may hold anything
 *     x[i,j,k] = x[i,j,k] + dt_T * g
 *     with TPG_AB2_STORE_PREVIOUS:  Gm[i,j,k] = Gn[i,j,k]       the bits of Gn; Gm may be written without being read
 *
 * Arrays
 * - `u` at (Face, Center, Center) and `v` at (Center, Face, Center), their tendencies `Gu_n`, `Gv_n`, `Gu_m`, `Gv_m`, and the `fields`,
 *   `Gn`, `Gm` of tpg_ab2_step_fields: padded parents of ONE geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
 * - `GU`, `GV`: 2-D padded planes of `(Ny + 2 Hy2) x (Nx + 2 Hx)`: the same `Hx`, so the same row pitch as the 3-D fields, and THEIR OWN
 *   north / south halo `Hy2` >= 0 (the free surface's fields live on the extended-halo grid), exactly as Ubar / Vbar of tpg_barotropic_mode.
 * - `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]` in the field type, as in tpg_w_from_continuity.
 * - `n_fc`, `n_cf`: NULL, or the (Face, Center) / (Center, Face) count planes of tpg_immersed_column_counts, Ny x Nx int32.
 * Neither call has a stencil: every halo width >= 0 is accepted, no halo cell of any array is read, only interior cells are written.
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.  Element offsets are
 * 64-bit.  Every check precedes any launch.
 *
 * tpg_ab2_step_velocities.  The rule on u with Gu_n, Gu_m and on v with Gv_n, Gv_m.  Where GU is given it also gets the forcing of the
 * sub-cycle, the column integral of the masked g, in the fixed order k = 1..Nz:
 *     ĝ_k = +0 where k <= min(max(n_fc[i,j], 0), Nz) (the peripheral nodes; n_fc NULL: nowhere), g otherwise
 *     GU[i,j] = dz_c[1] * ĝ_1;     for k = 2..Nz:  GU[i,j] = GU[i,j] + dz_c[k] * ĝ_k
 * and GV from v's g with n_cf likewise.  The first term is the product itself, and the products with +0 are carried out like the others.
 * The velocity itself is stepped with the unmasked g on every interior node: its mask is the correction's, later in the step.  A work item
 * owns one chunk of columns and walks ALL levels with the running integral in registers (level segments would re-associate the sum); it
 * stores u, and Gu_m under TPG_AB2_STORE_PREVIOUS, at its own cells only, so the in-place forms have no race.  ONE launch does both fields.
 * A field's whole group (u, Gu_n, Gu_m, GU) or (v, Gv_n, Gv_m, GV) may be NULL together, not both.  GU / GV may each be NULL: the step
 * without the integral.  Gu_m / Gv_m may be NULL only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear.
 * TPG_ERR_INVALID_ARGUMENT for a NULL required pointer, a half-given group, a null dz_c with GU or GV given, an unknown ft, unknown flag
 * bits, a pointer off its element or int32 alignment, Hy2 < 0, any written array (u, v, Gu_m / Gv_m under TPG_AB2_STORE_PREVIOUS, GU, GV)
 * overlapping any other array of the call (Gu_n == Gu_m included); TPG_ERR_UNSUPPORTED for more work items than 32 bits index. */
int tpg_ab2_step_velocities(void *u, void *v, const void *Gu_n, const void *Gv_n, void *Gu_m, void *Gv_m, void *GU, void *GV,
                            const void *dz_c, const int32_t *n_fc, const int32_t *n_cf, double dt, double chi, int flags,
                            int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int Hy2, int ft, void *stream);

/* tpg_ab2_step_fields.  The same rule on `n` <= TPG_MAX_FIELDS fields of one geometry -- the tracers: fields[f] with Gn[f], Gm[f].  No
 * integral, no mask.  ONE launch for all fields, one field per grid.y; a work item is one chunk x a segment of consecutive levels.
 * Gm (the table, or an entry) may be NULL only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear.
 * The checks of tpg_ab2_step_velocities, per field (the message names the field's index), and: TPG_ERR_INVALID_ARGUMENT for a null table,
 * n < 1 or n > TPG_MAX_FIELDS. */
int tpg_ab2_step_fields(void *const fields[], const void *const Gn[], void *const Gm[], int n, double dt, double chi, int flags,
                        int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_TIMESTEP_H */
