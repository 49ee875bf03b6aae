"""Host reference of the device reductions (tpg_field_extrema, tpg_cell_advection_timescale) in numpy, written from the rules.

field_extrema: over the interior i = 1..Nx, j = 1..Ny, k = 1..Nz' of a padded parent, (min c, max c, max |c|) widened to float64; np.min /
np.max propagate a NaN, as Julia's minimum / maximum do; an empty set gives (+inf, -inf, -inf).  With the NotImmersed condition the nodes
that mask_immersed_field! writes are left out [recalled; parity unpinned on nodes that are peripheral through the domain's own walls
only]: they come from immersed_ref.peripheral (the predicate), or from a count plane by the consequence the kernels use -- a z-Center field's
k <= n, a z-Face field's k <= min(n + 1, Nzg); a z-Face field's top level Nzg + 1 is never left out.

cell_advection_timescale [recalled: Oceananigans' rule; parity unpinned]: for every interior cell, in the field type, left to right,
    s = |u[i,j,k]| / dx_fc[i,j] + |v[i,j,k]| / dy_cf[i,j] + |w[i,j,k]| / dz_f[k]        tau = 1 / s
and the result is np.min(tau) over the counted cells (NaN if any is NaN; +inf if every s is 0 or no cell is counted), widened to float64.
With n_cc, cells k <= n_cc[i, j] are left out.  u, v: Nz levels; w: Nz + 1, of which levels 1..Nz are read.
Arrays are the padded parents, indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1]; locations are 0 (Center) / 1 (Face)."""
import numpy as np

from immersed_ref import peripheral


def interior(parent, size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert parent.shape == (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (parent.shape, size, halo)
    return parent[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]


def excluded_nodes(ina, loc, grid_size):
    """the nodes of a field at `loc` that the NotImmersed condition leaves out, (Nz', Ny, Nx) bool, from the predicate: Nz' = Nz for a
    z-Center field, Nz + 1 for a z-Face field, whose top level is counted"""
    Nx, Ny, Nz = grid_size
    per = peripheral(ina, loc, grid_size)
    if loc[2]:
        per = np.concatenate([per, np.zeros((1, Ny, Nx), dtype=bool)])
    return per


def excluded_from_plane(plane, zloc, nz_field):
    """the same set from the count plane of the field's (x, y) location: 1-based k <= min(n + zloc, nz_field - zloc)"""
    k = np.arange(1, nz_field + 1)[:, None, None]
    return k <= np.minimum(plane + zloc, nz_field - zloc)[None]


def field_extrema(parent, size, halo, excluded=None):
    """(min, max, max|c|) as float64 over the interior of `parent`; `size` is the FIELD's (its own level count)"""
    inner = interior(parent, size, halo)
    vals = inner.ravel() if excluded is None else inner[~excluded]
    if vals.size == 0:
        return (np.inf, -np.inf, -np.inf)
    return (np.float64(np.min(vals)), np.float64(np.max(vals)), np.float64(np.max(np.abs(vals))))


def cell_timescales(u, v, w, dx_fc, dy_cf, dz_f, size, halo):
    """tau of every interior cell, (Nz, Ny, Nx), in the field type"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    T = u.dtype
    assert v.dtype == T and w.dtype == T and dx_fc.dtype == T and dy_cf.dtype == T and dz_f.dtype == T and dz_f.shape == (Nz,)
    iu, iv = interior(u, size, halo), interior(v, size, halo)
    iw = interior(w, (Nx, Ny, Nz + 1), halo)[:Nz]                  # w's level Nz + 1 is not read
    dx = dx_fc[Hy:Hy + Ny, Hx:Hx + Nx][None]
    dy = dy_cf[Hy:Hy + Ny, Hx:Hx + Nx][None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.abs(iu) / dx + np.abs(iv) / dy + np.abs(iw) / dz_f[:, None, None]     # left to right
        tau = T.type(1) / s
    assert tau.dtype == T
    return tau


def cell_advection_timescale(u, v, w, dx_fc, dy_cf, dz_f, size, halo, n_cc=None):
    tau = cell_timescales(u, v, w, dx_fc, dy_cf, dz_f, size, halo)
    if n_cc is not None:
        tau = tau[~excluded_from_plane(n_cc, 0, size[2])]
    if tau.size == 0:
        return np.inf
    return np.float64(np.min(tau))


def same(a, b):
    """the comparison of the GPU tests: bit for bit, NaN-ness included; zeros compare by == (the sign of a zero extremum is not specified)"""
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if a == 0 and b == 0:
        return True
    return a.tobytes() == b.tobytes()
