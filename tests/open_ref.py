"""Host reference of the Open (impenetrable) south / bottom / top face write (tpg_fill_open_faces), shared by the CPU and GPU tests.

The rule [recalled: Oceananigans' fill_open_boundary_regions!, parity unpinned], 1-based on a numpy parent [k, j, i] of shape
(Nz+2Hz, Ny+2Hy, Nx+2Hx), Nz the field's own level count:
    south   c[i, 1, k]  = v     k = 1..Nz      a field at (Center, Face, Center)
    bottom  c[i, j, 1]  = v     j = 1..Ny      a field at (Center, Center, Face)
    top     c[i, j, Nz] = v     j = 1..Ny      a field at (Center, Center, Face)
The boundary face itself (an interior cell) is written, no halo cell; it is the first pass of the fill.

A side spec is None, "flux", (VALUE / GRADIENT, condition) as in value_gradient_ref.py, or (OPEN, condition) with the condition an FT scalar
or an FT array: south (Nz, Nx+2Hx), bottom / top (Ny+2Hy, Nx+2Hx) of which rows j = 1..Ny are read.
"""
import numpy as np

import value_gradient_ref as vg

OPEN = "open"


def is_open(spec):
    return isinstance(spec, tuple) and spec[0] == OPEN


def _cond(spec):
    return spec[1] if is_open(spec) else None


def _not_open(spec):
    return None if is_open(spec) else spec


def open_faces(a, size, halo, south, bottom, top, cols=None):
    """the face write; south / bottom / top: None or the condition (scalar or array); cols: slice of parent columns (None = whole rows).
    South first, then bottom and top: a cell that south and a z side both own takes the z side's value."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    cols = slice(None) if cols is None else cols
    rows = slice(Hy, Hy + Ny)

    def take(cond, r):
        cond = np.asarray(cond, dtype=a.dtype)
        return cond if cond.ndim == 0 else cond[r, cols]

    if south is not None:
        a[Hz:Hz + Nz, Hy, cols] = take(south, slice(None))
    if bottom is not None:
        a[Hz, rows, cols] = take(bottom, rows)
    if top is not None:
        a[Hz + Nz - 1, rows, cols] = take(top, rows)
    return a


def oceananigans_sequence_open(oracle, a, xl, yl, sg, size, halo, south, bottom, top, dy_row, dz):
    """Oceananigans' order as value_gradient_ref.oceananigans_sequence models it, with the open write put in front: open write on
    i = 1..Nx -> zipper -> south on i = 1..Nx -> bottom / top over the padded plane -> periodic x"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    open_faces(a, size, halo, _cond(south), _cond(bottom), _cond(top), slice(Hx, Hx + Nx))
    return vg.oceananigans_sequence(oracle, a, xl, yl, sg, size, halo, _not_open(south), _not_open(bottom), _not_open(top), dy_row, dz)


def library_sequence_open(oracle, a, xl, yl, sg, size, halo, south, bottom, top, dy_row, dz, horizontal=True):
    """The library's order: the open write over whole padded rows -> the whole horizontal fill -> Value / Gradient south -> no-flux
    mirror -> Value / Gradient bottom / top"""
    open_faces(a, size, halo, _cond(south), _cond(bottom), _cond(top))
    return vg.post_pass_sequence(oracle, a, xl, yl, sg, size, halo, _not_open(south), _not_open(bottom), _not_open(top), dy_row, dz,
                                 horizontal=horizontal)
