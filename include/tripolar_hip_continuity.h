/*
 * tripolar_hip_continuity.h -- C ABI of libtripolar_hip_continuity.so: the horizontal divergence and w from continuity on the fields of a
 * TripolarGrid for MI355X (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word:
 * extern "C", plain pointers, caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns
 * TPG_OK, a negative tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, as libtripolar_hip_operators.so (include/tripolar_hip_operators.h) is: the export lists of the other two are pinned.
 * The libraries share no state: tpg_continuity_last_error() returns the thread-local message of the last failure of a call INTO THIS
 * LIBRARY on this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_CONTINUITY_H
#define TRIPOLAR_HIP_CONTINUITY_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_continuity_last_error(void);

/* ---- w from continuity and the horizontal divergence ------------------------------------------------
 * What a hydrostatic model diagnoses from u and v after each velocity update, before the time-step wizard and the output writer that the
 * reference's drivers point at model.velocities, w included.
 * [recalled: Oceananigans' `div_xyᶜᶜᶜ` and `_compute_w_from_continuity!`; parity unpinned, like every operator here.]
 *
 * Fields
 * - `u` at (Face, Center, Center) and `v` at (Center, Face, Center): padded parents of geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
 * - `w` at (Center, Center, Face): a padded parent with `Nz + 1` interior levels, `Nz + 1 + 2Hz` planes, same `sx`, `sy`.
 * - `div` at (Center, Center, Center): a parent like u's.
 * Metrics
 * - The grid's padded planes `dy_fc` (`Δyᶠᶜᵃ`), `dx_cf` (`Δxᶜᶠᵃ`), `az_cc` (`Azᶜᶜᵃ`), halos built.
 * - `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]` in the field type.
 * Arithmetic, for every interior column `i = 1..Nx`, `j = 1..Ny`, in the field type, in exactly this order, no contraction, every operation
 * one correctly rounded IEEE operation:
 *     w[i,j,1] = +0
 *     for k = 1..Nz, d = dz_c[k]:
 *         fe = (dy_fc[i+1,j] * d) * u[i+1,j,k]        fw = (dy_fc[i,j] * d) * u[i,j,k]
 *         fn = (dx_cf[i,j+1] * d) * v[i,j+1,k]        fs = (dx_cf[i,j] * d) * v[i,j,k]
 *         V  = az_cc[i,j] * d
 *         div[i,j,k] = (1 / V) * ((fe - fw) + (fn - fs))
 *         w[i,j,k+1] = w[i,j,k] - d * div[i,j,k]
 * - `fe` of column `i` IS `fw` of column `i+1`. `fn` of row `j` IS `fs` of row `j+1`. Each is formed once.
 * - Cells read: `u[1..Nx+1, 1..Ny, 1..Nz]` and the same cells of `dy_fc`; `v[1..Nx, 1..Ny+1, 1..Nz]` and the same cells of `dx_cf`;
 *   `az_cc` interior; `dz_c`.
 * - That is one halo column to the east and one halo row to the north, so `Hx ≥ 1` and `Hy ≥ 1`. THE CALLER HAS FILLED THE HALOS OF u AND v.
 * - On a latitude band `Ny` is the band's row count and row `Ny+1` the exchanged (or, on the last band, folded) north halo row.
 * - Only interior cells of `w` (levels `1..Nz+1`) and `div` are written.
 * - `V = 0` divides by it, as the rule says.
 *
 * ONE launch.  `w` or `div` may be NULL, not both: with w == NULL nothing carries from level to level, with div == NULL the divergence lives
 * in registers only.  Nz is the GRID's level count: u, v and div have Nz levels, w has Nz + 1.
 * n_cc: NULL, or the (Center, Center) count plane of tpg_immersed_column_counts, Ny x Nx int32.  The scan runs on the unmasked values
 * (levels under the mask ARE read: a model's u and v are masked there); where they are stored, div nodes k <= n and w faces
 * k <= min(n + 1, Nz) get mask_value (converted once to the field type) instead: bit for bit what the call with n_cc = NULL leaves after
 * tpg_mask_immersed_fields on w (that plane, TPG_FACE) and on div (that plane, TPG_CENTER).  mask_value is not read when n_cc is NULL.
 * A work item keeps the metrics of a few rows of one chunk and the running w in registers and walks ALL levels (the recurrence forbids level
 * segments); 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned chunks otherwise.  Float32 and Float64, every halo
 * width >= 1, every pointer aligned to its element type; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable
 * into a HIP graph.  Element offsets are 64-bit.
 * Aliasing: w's and div's parents (each with its own plane count) may overlap neither u's nor v's nor each other's; u and v may be one array.
 * Every check precedes any launch: TPG_ERR_INVALID_ARGUMENT for a null u, v, metric or dz_c pointer, w and div both NULL, an unknown ft, a
 * pointer off its element alignment (n_cc: int32), an overlap as above; TPG_ERR_UNSUPPORTED for Hx < 1, Hy < 1, or more work items than
 * 32 bits index. */
int tpg_w_from_continuity(const void *u, const void *v, void *w, void *div,
                          const void *dy_fc, const void *dx_cf, const void *az_cc, const void *dz_c,
                          const int32_t *n_cc, double mask_value,
                          int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_CONTINUITY_H */
