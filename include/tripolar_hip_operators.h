/*
 * tripolar_hip_operators.h -- C ABI of libtripolar_hip_operators.so: diagnostic operators on the fields of a TripolarGrid for MI355X
 * (gfx950), beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word: extern "C", plain pointers,
 * caller-owned DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative
 * tpg_status or a positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own: libtripolar_hip.so exports exactly the symbols of tripolar_hip.h, which stand for the reference's own interfaces
 * and whose list is pinned; the operators below stand for Oceananigans operators that the reference's model DRIVERS call.  The two
 * libraries share no state: tpg_operators_last_error() returns the thread-local message of the last failure of a call INTO THIS LIBRARY
 * on this thread (tpg_last_error() of libtripolar_hip.so does not see it); status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_OPERATORS_H
#define TRIPOLAR_HIP_OPERATORS_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_operators_last_error(void);

/* ---- the vertical vorticity at (Face, Face, Center) ------------------------------------------------
 * What the reference's model drivers create with VerticalVorticityField(model) (examples/bickley_jet.jl:57;
 * examples/distributed_bickley_jet.jl:59) and write beside the velocities and tracers on every output (:79 / :83); the field whose
 * fold src/zipper_boundary_condition.jl:154-155 was written for.
 *
 * tpg_vertical_vorticity: Oceananigans' vertical vorticity operator at (Face, Face, Center) [recalled; parity unpinned -- the rule is stated
 * here and in tests/vorticity_ref.py].  For every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz, in the field type, in exactly this order,
 * no contraction, every operation one correctly rounded IEEE operation:
 *     a = dy_cf[i,j] * v[i,j,k]     b = dy_cf[i-1,j] * v[i-1,j,k]     c = dx_fc[i,j] * u[i,j,k]     d = dx_fc[i,j-1] * u[i,j-1,k]
 *     zeta[i,j,k] = ((a - b) - (c - d)) / az_ff[i,j]
 * u at (Face, Center, Center), v at (Center, Face, Center), zeta at (Face, Face, Center): three padded parents of ONE geometry
 * (Nx, Ny, Nz, Hx, Hy, Hz) and one element type.  dx_fc, dy_cf, az_ff: the grid's padded 2-D metrics (Ny+2Hy) x (Nx+2Hx), halos built.
 * Cells read: u[i, j-1..j, k] and v[i-1..i, j, k] (and dx_fc / dy_cf at the same (i, j)), az_ff[i, j]: column i = 0 and row j = 0 are halo
 * cells, so Hx >= 1 and Hy >= 1, and THE CALLER HAS FILLED THE HALOS OF u AND v, as for any stencil.  On a latitude band Ny is the band's
 * row count and row 0 the exchanged south halo row; nothing else changes.  Only INTERIOR cells of zeta are written: its halos are the
 * fill's (tpg_fill_halo_regions with xloc = yloc = TPG_FACE, sign +1).  An az_ff of 0 divides by it, as the rule says (Inf or NaN).
 * n_ff: NULL, or the (Face, Face) count plane of tpg_immersed_column_counts -- nodes k <= n_ff[i,j] get mask_value (converted once to the
 * field type) and nothing is computed there: bit for bit what the call with n_ff = NULL followed by tpg_mask_immersed_fields on zeta
 * (that plane, TPG_CENTER, mask_value) leaves.  mask_value is not read when n_ff is NULL.
 * ONE launch; a work item keeps the metrics of a few rows of one chunk in registers and walks the levels innermost (the metric planes are
 * not re-fetched per level); 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned chunks otherwise.  Float32 and
 * Float64, every halo width >= 1, every pointer aligned to its element type; no atomics, nothing allocated, asynchronous on `stream` (no host
 * wait), capturable into a HIP graph.
 * Aliasing: zeta's parent may overlap neither u's nor v's (a node reads cells that its neighbours' nodes would overwrite); u and v may be
 * one array.  Every check precedes any launch: TPG_ERR_INVALID_ARGUMENT for a null pointer (n_ff may be NULL), an unknown ft, a pointer
 * off its element alignment (n_ff: int32), zeta's parent overlapping u's or v's; TPG_ERR_UNSUPPORTED for Hx < 1, Hy < 1, or more work items
 * than 32 bits index.  Element offsets are 64-bit. */
int tpg_vertical_vorticity(const void *u, const void *v, void *zeta,
                           const void *dx_fc, const void *dy_cf, const void *az_ff,
                           const int32_t *n_ff, double mask_value,
                           int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_OPERATORS_H */
