"""Host reference of the no-flux south / bottom / top halo fill (tpg_fill_bounded_halos), shared by the CPU and GPU tests.

1-based Oceananigans indexing on a numpy parent [k, j, i] of shape (Nz+2Hz, Ny+2Hy, Nx+2Hx):
    south   c[i, 1-j, k]  = c[i, j, k]        j = 1..Hy, k = 1..Nz
    bottom  c[i, j, 1-k]  = c[i, j, k]        k = 1..Hz, every (i, j) of the padded plane
    top     c[i, j, Nz+k] = c[i, j, Nz+1-k]   k = 1..Hz, every (i, j) of the padded plane
"""
import numpy as np

SOUTH, BOTTOM, TOP = 1, 2, 4


def south_mirror(a, size, halo, cols=None):
    """south rows of the interior levels; cols: slice of parent columns (None = the whole padded row)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    cols = slice(None) if cols is None else cols
    for j in range(1, Hy + 1):
        a[Hz:Hz + Nz, Hy - j, cols] = a[Hz:Hz + Nz, Hy + j - 1, cols]
    return a


def z_mirror(a, size, halo, bottom=True, top=True):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    for k in range(1, Hz + 1):
        if bottom:
            a[Hz - k] = a[Hz + k - 1]
        if top:
            a[Hz + Nz + k - 1] = a[Hz + Nz - k]
    return a


def bounded_sequence(oracle, a, xl, yl, sg, size, halo, sides):
    """The first order of the issue: zipper over k = 1..Nz -> south mirror on i = 1..Nx -> bottom / top over the padded plane ->
    periodic x (Oceananigans' own pass order for a Flux-bounded field, with the reference's zipper as the north side)."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    oracle.zipper_fill(a, xl, yl, sg, size, halo)
    if sides & SOUTH:
        south_mirror(a, size, halo, slice(Hx, Hx + Nx))
    z_mirror(a, size, halo, bool(sides & BOTTOM), bool(sides & TOP))
    oracle.periodic_x_fill(a, size, halo)
    return a


def post_pass_sequence(oracle, a, xl, yl, sg, size, halo, sides):
    """The library's order: the whole horizontal fill, then south over whole padded rows, then bottom / top."""
    oracle.fill_halo_regions(a, xl, yl, sg, size, halo)
    if sides & SOUTH:
        south_mirror(a, size, halo)
    z_mirror(a, size, halo, bool(sides & BOTTOM), bool(sides & TOP))
    return a


def random_field(rng, size, halo, dtype):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return rng.uniform(-1, 1, (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)).astype(dtype)
