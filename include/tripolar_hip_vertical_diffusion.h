/*
 * tripolar_hip_vertical_diffusion.h -- C ABI of libtripolar_hip_vertical_diffusion.so: the vertically implicit diffusion step of a
 * hydrostatic model, a batched tridiagonal solve along z with one system per column, on the fields of a TripolarGrid for MI355X (gfx950),
 * beside libtripolar_hip.so (include/tripolar_hip.h), whose conventions hold here word for word: extern "C", plain pointers, caller-owned
 * DEVICE memory, padded parent arrays with i fastest, `ft` = TPG_F32 / TPG_F64, every call returns TPG_OK, a negative tpg_status or a
 * positive hipError_t, asynchronous on `stream`, capturable into a HIP graph, no environment variable read.
 *
 * A library of its own, the fifteenth, as the other operator libraries are: the export lists of the other fourteen are pinned.  The
 * libraries share no state: tpg_vertical_diffusion_last_error() returns the thread-local message of the last failure of a call INTO THIS
 * LIBRARY on this thread; status codes and their strings are tripolar_hip.h's.
 */
#ifndef TRIPOLAR_HIP_VERTICAL_DIFFUSION_H
#define TRIPOLAR_HIP_VERTICAL_DIFFUSION_H

#include "tripolar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *tpg_vertical_diffusion_last_error(void);

/* `kappa_form` of tpg_vertical_implicit_diffusion: where the diffusivity at the faces comes from.  Every other value is refused with
 * TPG_ERR_UNSUPPORTED, the message names it. */
#define TPG_KAPPA_CONSTANT 0 /* `kappa` is NULL: T(kappa_value) on every face */
#define TPG_KAPPA_PROFILE 1  /* `kappa`: Nz + 1 device values at the faces 1..Nz+1 */
#define TPG_KAPPA_FIELD 2    /* `kappa`: a padded parent of the call's geometry at (the fields' horizontal location, Face): face k at plane Hz + k - 1 */

/* `path` of tpg_vertical_implicit_diffusion: where the intermediates of the two sweeps live.  Every path gives the same bits.  Every other
 * value is refused with TPG_ERR_UNSUPPORTED, the message names it. */
#define TPG_VDIFF_AUTO 0     /* with `scratch`: STREAMED, which the measurements favour; without: ON_CHIP, or refused beyond its bound */
#define TPG_VDIFF_ON_CHIP 1  /* t in LDS, [level][column]: nothing but the fields is written to memory; `scratch` may be NULL */
#define TPG_VDIFF_STREAMED 2 /* t in `scratch`: any Nz */

/* The greatest Nz the on-chip path serves for `n` fields of type `ft` (it does not grow with n); < 0: a tpg_status (an unknown ft, n < 1 or
 * n > TPG_MAX_FIELDS: TPG_ERR_INVALID_ARGUMENT). */
int tpg_vertical_diffusion_on_chip_levels(int n, int ft);

/* ---- the vertically implicit diffusion step: Oceananigans' implicit_step! ---------------------------------------------------------------
 * With a closure VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), nu, kappa) the model solves, right after the AB2 update of
 * u, v and every tracer, (1 - dt d/dz kappa d/dz) phi = f in every column: a tridiagonal system.  ONE CALL IS ONE MATRIX PER COLUMN AND UP TO
 * TPG_MAX_FIELDS RIGHT-HAND SIDES: the `n` fields are padded parents of one geometry at ONE horizontal location, they share `kappa`,
 * `counts` and `dt`, and they are solved IN PLACE.  A model makes three calls: u with nu and n_fc, v with nu and n_cf, the tracers with
 * kappa and n_cc.
 * [recalled: Oceananigans' ivd_upper_diagonal / ivd_lower_diagonal / ivd_diagonal, kappa_dz2, and solve_batched_tridiagonal_system_z!;
 * parity unpinned, like every operator here]
 *
 * THE RULE, for every interior column (i, j).  It is evaluated in the field type T, in exactly this order, with no contraction.  Every
 * operation is one correctly rounded IEEE operation.  k0 = 1 without `counts`; with them k0 = min(max(counts[j,i], 0), Nz) + 1.  Face k lies
 * between the cells k-1 and k.
 *     dtT = T(dt), one = T(1)
 *     for every face k = k0+1 .. Nz:
 *         up[k-1] = -(dtT * ((kappa[k] / dz_c[k-1]) / dz_f[k]))        the coefficient of phi[k]   in row k-1
 *         lo[k]   = -(dtT * ((kappa[k] / dz_c[k])   / dz_f[k]))        the coefficient of phi[k-1] in row k
 *     diag[k] = (one - up[k]) - lo[k]; the term of a closed face (below k0, above Nz) is omitted, not replaced by a zero:
 *               one - up[k0] in the bottom row, one - lo[Nz] in the top row, one where k0 = Nz
 *     beta = diag[k0];  phi[k0] = f[k0] / beta
 *     for k = k0+1 .. Nz, in this order:
 *         t[k] = up[k-1] / beta;   beta = diag[k] - lo[k] * t[k]
 *         phi[k] = (|beta| > T(10) * eps(T)) ? (f[k] - lo[k] * phi[k-1]) / beta : f[k]
 *     for k = Nz-1 .. k0, in this order:   phi[k] = phi[k] - t[k+1] * phi[k+1]
 * - f is what the field held on entry.  eps(T) is 2^-52 / 2^-23.  A NaN beta takes the second arm of the select.
 * - Signs.  Leading minus signs are sign flips.
 * - Nz = 1 returns f / one.
 * - No boundary flux enters here: the faces 1 and Nz + 1 carry none (Oceananigans puts them into the explicit tendency).
 * - Mask.  With `counts` (an Ny x Nx int32 plane of tpg_immersed_column_counts at the fields' horizontal location) the cells k < k0 receive
 *   T(mask_value): what tpg_mask_immersed_fields leaves.  A column with k0 > Nz is all mask.  This is the system of the wet levels alone;
 *   Oceananigans' identity rows under the bottom differ from it in signs of zero and where a non-finite value sits under the bottom.
 * - kappa, by `kappa_form`: TPG_KAPPA_CONSTANT, `kappa` must be NULL; TPG_KAPPA_PROFILE, Nz + 1 values, of which the faces 2..Nz are
 *   loaded; TPG_KAPPA_FIELD, a padded parent, loaded at the planes of the faces 2..Nz of the node's own column.  In every form only the
 *   faces k0+1..Nz enter the result: the planes of the faces 1 and Nz + 1 and every halo cell are never read.  The three forms give the same
 *   bits on equal values.
 * - dz_c: Nz values, dz_f: Nz + 1 values, in the field type: the tables of z_center_spacings and z_all_face_spacings.  Of dz_f only the faces
 *   k0+1..Nz enter the result (dz_f[1] and dz_f[Nz+1] never do).
 * - Halos.  No halo cell of any array is read or written: every halo width >= 0 that the geometry check admits is accepted (each at most
 *   the size in its direction horizontally).  The rule is column-local: a latitude band gives the rows of the global call.
 * - Written.  Only interior cells of the fields and, on the streamed path, of `scratch`.
 *
 * WHERE THE INTERMEDIATES LIVE.  The back sweep needs t[k+1], shared by the n fields, and the forward phi[k] of every field.  The forward
 * phi goes to the field's own cells (ordinary, cacheable stores), and the back sweep reads it there again: a work item re-reads only what
 * it wrote itself, so nothing is synchronised.  t goes, by `path`, to LDS laid out [level][column] (TPG_VDIFF_ON_CHIP: Nz at most
 * tpg_vertical_diffusion_on_chip_levels(n, ft); `scratch` may be NULL) or to `scratch` (TPG_VDIFF_STREAMED: a caller-owned padded parent of
 * the call's geometry and type, required; only its interior cells are written, its contents on return are unspecified).  One kernel template
 * with the two storage policies: the same sequence of operations, the same bits.  TPG_VDIFF_AUTO takes the streamed path when `scratch`
 * is given (measured at 3600 x 1800 x 75: the on-chip path holds few waves per CU at that depth and is the slower one); without `scratch` it
 * takes the on-chip path or refuses.
 *
 * Float32 and Float64, every pointer aligned to its element type; 16-B chunks where rows and pointers sit on the 16-B grid, element-aligned
 * chunks otherwise; ONE launch; no atomics, nothing allocated, asynchronous on `stream` (no host wait), capturable into a HIP graph.
 * Element offsets are 64-bit.  Every check precedes any launch.
 *
 * Out of this call: interpolating a (Center, Center, Face) diffusivity to the columns of u and v is the caller's job (the FIELD form takes
 * kappa at the fields' own horizontal location); the explicit diffusive tendency and boundary fluxes; computing kappa.
 *
 * Refusals, in this order, each with its own message:
 *  1. the geometry checks every entry point shares (unknown ft, an invalid size or halo: TPG_ERR_INVALID_ARGUMENT; odd Nx:
 *     TPG_ERR_ODD_NLAMBDA; a halo larger than the size, a plane past 32-bit indexing: TPG_ERR_UNSUPPORTED);
 *  2. n < 1 or n > TPG_MAX_FIELDS, a null `fields` or a null entry of it: TPG_ERR_INVALID_ARGUMENT;
 *  3. a `kappa_form` other than the three above, then a `path` other than the three above: TPG_ERR_UNSUPPORTED, the message names the value;
 *  4. null combinations, TPG_ERR_INVALID_ARGUMENT: `kappa` given with TPG_KAPPA_CONSTANT; `kappa` missing with TPG_KAPPA_PROFILE or
 *     TPG_KAPPA_FIELD; a null dz_c or dz_f; TPG_VDIFF_STREAMED without `scratch`;
 *  5. a dt, or with TPG_KAPPA_CONSTANT a kappa_value, that is not finite: TPG_ERR_INVALID_ARGUMENT;
 *  6. a pointer off its element alignment, `counts` off int32 alignment: TPG_ERR_INVALID_ARGUMENT;
 *  7. overlaps, TPG_ERR_INVALID_ARGUMENT: a field overlapping another field, `scratch` or a TPG_KAPPA_FIELD kappa; `scratch` overlapping
 *     `kappa`;
 *  8. Nz beyond tpg_vertical_diffusion_on_chip_levels(n, ft) with TPG_VDIFF_ON_CHIP, or with TPG_VDIFF_AUTO without `scratch`:
 *     TPG_ERR_UNSUPPORTED, the message states the bound;
 *  9. more work items than 32 bits index: TPG_ERR_UNSUPPORTED.
 * Everything else is served, down to (Nx, Ny, Nz) = (2, 1, 1) at halo (1, 1, 1). */
int tpg_vertical_implicit_diffusion(void *const fields[], int n, const void *kappa, double kappa_value, int kappa_form,
                                    const void *dz_c, const void *dz_f, const int32_t *counts, double mask_value, double dt,
                                    void *scratch, int path, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPOLAR_HIP_VERTICAL_DIFFUSION_H */
