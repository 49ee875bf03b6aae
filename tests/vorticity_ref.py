"""Host reference of the vertical vorticity at (Face, Face, Center) in numpy, on padded parents.

The rule [recalled: Oceananigans' ζ₃ᶠᶠᶜ; its source is not at hand, parity unpinned -- this file and include/tripolar_hip.h state it].  For every
interior node i = 1..Nx, j = 1..Ny, k = 1..Nz, in the fields' element type, in exactly this order, no contraction:
    a = dy_cf[i,j]   * v[i,j,k]        b = dy_cf[i-1,j] * v[i-1,j,k]
    c = dx_fc[i,j]   * u[i,j,k]        d = dx_fc[i,j-1] * u[i,j-1,k]
    zeta[i,j,k] = ((a - b) - (c - d)) / az_ff[i,j]
u at (Face, Center, Center), v at (Center, Face, Center), zeta at (Face, Face, Center): parents of one geometry, indexed
[k + Hz - 1, j + Hy - 1, i + Hx - 1]; the metrics are padded planes indexed [j + Hy - 1, i + Hx - 1].  Every operation is one correctly rounded
IEEE operation of the element type, which numpy's elementwise arithmetic in that dtype is too: the reference is exact, comparisons are bit for
bit.  Only the interior of zeta is written.  With a (Face, Face) count plane n_ff (Ny, Nx), nodes k <= n_ff[i,j] hold the mask value instead."""
import numpy as np

# the stencil, derived from the rule above: (array, di, dj) of every cell a node (i, j, k) reads
STENCIL = (("v", 0, 0), ("dy_cf", 0, 0), ("v", -1, 0), ("dy_cf", -1, 0),
           ("u", 0, 0), ("dx_fc", 0, 0), ("u", 0, -1), ("dx_fc", 0, -1), ("az_ff", 0, 0))


def _win(p, size, halo, di=0, dj=0):
    """the cells (i + di, j + dj) for i = 1..Nx, j = 1..Ny of a padded plane or parent (all interior levels of a parent)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    ys, xs = slice(Hy + dj, Hy + dj + Ny), slice(Hx + di, Hx + di + Nx)
    return p[ys, xs] if p.ndim == 2 else p[Hz:Hz + Nz, ys, xs]


def interior_vorticity(u, v, dx_fc, dy_cf, az_ff, size, halo):
    """zeta on the interior, (Nz, Ny, Nx), in the dtype of u"""
    T = u.dtype
    assert v.dtype == T and dx_fc.dtype == T and dy_cf.dtype == T and az_ff.dtype == T
    w = lambda p, di=0, dj=0: _win(p, size, halo, di, dj)
    with np.errstate(all="ignore"):
        a = w(dy_cf) * w(v)
        b = w(dy_cf, -1, 0) * w(v, -1, 0)
        c = w(dx_fc) * w(u)
        d = w(dx_fc, 0, -1) * w(u, 0, -1)
        z = ((a - b) - (c - d)) / w(az_ff)
    assert z.dtype == T
    return z


def vertical_vorticity(u, v, zeta, dx_fc, dy_cf, az_ff, size, halo, n_ff=None, mask_value=0.0):
    """the parent of zeta after the call: a copy of `zeta` with the interior replaced (halo cells untouched)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    z = interior_vorticity(u, v, dx_fc, dy_cf, az_ff, size, halo)
    if n_ff is not None:
        k = np.arange(1, Nz + 1)[:, None, None]
        z = np.where(k <= n_ff[None], u.dtype.type(mask_value), z)
    out = zeta.copy()
    out[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = z
    return out


def cells_read(size, halo):
    """boolean masks of the cells the rule reads, derived from STENCIL: {"u", "v": parent-shaped; "dx_fc", "dy_cf", "az_ff": plane-shaped}"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    plane, parent = (Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    read = {"u": np.zeros(parent, bool), "v": np.zeros(parent, bool),
            "dx_fc": np.zeros(plane, bool), "dy_cf": np.zeros(plane, bool), "az_ff": np.zeros(plane, bool)}
    for name, di, dj in STENCIL:
        _win(read[name], size, halo, di, dj)[...] = True
    return read


def same_bits(got, want):
    """bit for bit, NaNs compared by NaN-ness; returns the number of cells that differ"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    I = np.uint64 if got.dtype == np.float64 else np.uint32
    eq = (got.view(I) == want.view(I)) | (np.isnan(got) & np.isnan(want))
    return int((~eq).sum())
