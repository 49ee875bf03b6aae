"""What the tests of the diffusive tendency share (tests/test_diffusion_ref.py, tests/test_gpu_diffusion.py): the draw of a problem of
tests/diffusion_ref.py -- every array random in EVERY cell unless a test plants something --, and a bottom height with its halos filled as a
grid fills them, drawn so that every kind of column and of closed face occurs."""
import numpy as np

import diffusion_ref as R
from immersed_ref import column_counts, heights_of

F32, F64 = np.float32, np.float64
SENTINEL = -777.25


def z_centres(Nz, dtype):
    return np.linspace(-1, 0, 2 * Nz + 1)[1::2].astype(dtype)


def fold_partner(size, halo):
    """(j, i), 0-based interior indices: the cell whose value the fill leaves in row Ny + 1 above column i, as arrays over i"""
    from oracle import oracle
    (Nx, Ny, _), (Hx, Hy, _) = size, halo
    tag = np.zeros((1, Ny + 2 * Hy, Nx + 2 * Hx))
    tag[0, Hy:Hy + Ny, Hx:Hx + Nx] = 1000.0 * np.arange(Ny)[:, None] + np.arange(Nx)[None, :]
    oracle.fill_halo_regions(tag, 0, 0, 1, (Nx, Ny, 1), (Hx, Hy, 0))
    row = tag[0, Hy + Ny, Hx:Hx + Nx].astype(np.int64)
    return row // 1000, row % 1000


def bottom(size, halo, dtype, seed=0):
    """(h, zc, counts): a padded bottom-height plane with its halos filled (zipper north, periodic x; the south halo holds NaN: behind the
    wall), the Nz centres, and the four count planes of the FILLED h.  Where the shape has room: land at the columns 1 and Nx, land in row 1,
    land at the fold partner of a wet cell of row Ny, an isolated wet cell, an all-land column and a column with one wet cell"""
    from oracle import oracle
    (Nx, Ny, Nz), (Hx, Hy, _) = size, halo
    rng = np.random.default_rng([41 + seed, *size, *halo])
    zc = z_centres(Nz, dtype)
    c = rng.integers(0, Nz + 1, (Ny, Nx))
    roomy = Nx >= 8 and Ny >= 5
    if roomy:
        c[1:, 0] = Nz
        c[:-1, Nx - 1] = Nz
        c[0, 1:3] = Nz
        c[0, 3] = 0
        c[1:4, 2:5] = Nz                                           # an isolated wet cell at row 3, column 4 (1-based)
        c[2, 3] = 0
        c[1, 5] = Nz - 1
        pj, pi = fold_partner(size, halo)
        c[Ny - 1, 1], c[Ny - 1, Nx - 2] = 0, 0                     # row Ny comes out mirror-symmetric: both ends of the pair
        c[Ny - 2, 1] = 0                                           # and the cell south of it is wet
        c[pj[1], pi[1]] = Nz if (pj[1], pi[1]) not in ((Ny - 1, 1), (Ny - 1, Nx - 2)) else 0
    h = np.full((1, Ny + 2 * Hy, Nx + 2 * Hx), np.nan, dtype)
    h[0, Hy:Hy + Ny, Hx:Hx + Nx] = heights_of(c, zc, rng)
    oracle.fill_halo_regions(h, 0, 0, 1, (Nx, Ny, 1), (Hx, Hy, 0))
    h = h[0]
    h[:Hy] = np.nan                                                # never read behind the wall
    counts = column_counts(h, zc, size, halo, True)
    h.setflags(write=False)
    return h, zc, counts


def draw(size, halo, dtype, *, nfields=1, terms=R.HORIZONTAL | R.VERTICAL, mode=R.WRITE, form=R.CONSTANT, top=(), bottom_flux=(), masked=False,
         closed=False, loc="cc", seed=0, wall=True):
    """a problem of diffusion_ref: c, G (the sentinel in WRITE mode, random in ADD), the metrics and spacings in [0.5, 2], kappa in [0, 2],
    fluxes in [-1, 1].  `top`, `bottom_flux`: the indices of the fields that have a plane (an empty tuple: no table).  `masked`: the count
    plane at `loc` of the drawn bottom; `closed`: its bottom height"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng([*size, *halo, np.dtype(dtype).itemsize, seed])
    shape = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    plane = shape[1:]
    U = lambda lo, hi, s: rng.uniform(lo, hi, s).astype(dtype)     # noqa: E731
    c = [U(-1, 1, shape) for _ in range(nfields)]
    G = [U(-1, 1, shape) if mode == R.ADD else np.full(shape, SENTINEL, dtype) for _ in range(nfields)]
    metrics = {k: U(0.5, 2, plane) for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf", "az")}
    dz_c, dz_f = U(0.5, 2, Nz), U(0.5, 2, Nz + 1)
    dz_f[0] = dz_f[Nz] = np.nan                                    # the two boundary faces are never read
    if form == R.CONSTANT:
        kappa = 0.37
    elif form == R.PROFILE:
        kappa = U(0, 2, Nz + 1)
        kappa[0] = kappa[Nz] = np.nan
    else:
        kappa = np.full((Nz + 1 + 2 * Hz, *plane), np.nan, dtype)  # NaN in every halo cell and in the planes of the faces 1 and Nz + 1
        kappa[Hz + 1:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = U(0, 2, (max(Nz - 1, 0), Ny, Nx))

    def planes(which):
        if not len(which) and which != "all":
            return None
        out = []
        for q in range(nfields):
            if which == "all" or q in which:
                J = np.full(plane, np.nan, dtype)                  # only the interior is read
                J[Hy:Hy + Ny, Hx:Hx + Nx] = U(-1, 1, (Ny, Nx))
                out.append(J)
            else:
                out.append(None)
        return out
    h = zc = counts = None
    if masked or closed:
        hh, zz, cc = bottom(size, halo, dtype)
        counts = cc[loc] if masked else None
        if closed:
            h, zc = hh, zz
    return R.problem(c, G, terms, mode, size, halo, kappa_h=0.61, kappa_z=kappa, form=form, dz_c=dz_c, dz_f=dz_f, top=planes(top),
                     bottom=planes(bottom_flux), counts=counts, mask_value=0.0, h=h, zc=zc, wall=wall, **metrics)
