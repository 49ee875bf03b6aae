"""Host reference of the Value / Gradient south / bottom / top halo fill (tpg_fill_value_gradient_halos), shared by the CPU and GPU tests.

The rule [recalled: Oceananigans' fill_halo_regions_value_gradient.jl, parity unpinned], 1-based on a numpy parent [k, j, i] of shape
(Nz+2Hz, Ny+2Hy, Nx+2Hx), every operation in the field's type FT, in this order:
    south   c[i, 0, k]    = c[i, 1, k]  + D * (-d)   d = dy_cf[i, 1]
    bottom  c[i, j, 0]    = c[i, j, 1]  + D * (-d)   d = dz_bottom
    top     c[i, j, Nz+1] = c[i, j, Nz] + D * d      d = dz_top
D = (c[1] - v) / (d / 2) (top: (v - c[Nz]) / (d / 2)) for Value, D = g for Gradient.  Only the first halo point is written.

A side spec is None, "flux" (the no-flux mirror of bounded_ref.py) or (kind, condition) with kind VALUE / GRADIENT and the condition an
FT scalar or an FT array: south (Nz, Nx+2Hx), bottom / top (Ny+2Hy, Nx+2Hx).
"""
import numpy as np

from bounded_ref import south_mirror, z_mirror

VALUE, GRADIENT = 1, 2


def extrapolate(kind, c1, cond, d, upper):
    """the first halo point beyond c1 (the source cell), in c1's type; upper: the top side"""
    ft = c1.dtype.type
    cond, d = np.asarray(cond, dtype=c1.dtype), np.asarray(d, dtype=c1.dtype)
    if kind == VALUE:
        half = d / ft(2)
        grad = (cond - c1) / half if upper else (c1 - cond) / half
    elif kind == GRADIENT:
        grad = cond
    else:
        raise ValueError(kind)
    out = c1 + grad * d if upper else c1 + grad * (-d)
    assert out.dtype == c1.dtype
    return out


def _cols(cond, cols):
    cond = np.asarray(cond)
    return cond if cond.ndim == 0 else cond[..., cols]


def south_vg(a, size, halo, kind, cond, dy_row, cols=None):
    """row 0 of the interior levels from row 1; dy_row: parent row j = 1 of dy_cf; cols: slice of parent columns (None = whole rows)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    if Hy == 0:
        return a
    cols = slice(None) if cols is None else cols
    a[Hz:Hz + Nz, Hy - 1, cols] = extrapolate(kind, a[Hz:Hz + Nz, Hy, cols], _cols(cond, cols), np.asarray(dy_row)[cols][None, :], False)
    return a


def z_vg(a, size, halo, bottom, top, dz):
    """planes 0 and Nz+1 over the whole padded plane; bottom / top: (kind, condition) or None"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    if Hz == 0:
        return a
    if bottom is not None:
        a[Hz - 1] = extrapolate(bottom[0], a[Hz], bottom[1], dz[0], False)
    if top is not None:
        a[Hz + Nz] = extrapolate(top[0], a[Hz + Nz - 1], top[1], dz[1], True)
    return a


def _vg(spec):
    return spec if isinstance(spec, tuple) else None


def oceananigans_sequence(oracle, a, xl, yl, sg, size, halo, south, bottom, top, dy_row, dz):
    """Oceananigans' pass order: zipper over k = 1..Nz -> south on i = 1..Nx -> bottom / top over the padded plane -> periodic x"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    interior = slice(Hx, Hx + Nx)
    oracle.zipper_fill(a, xl, yl, sg, size, halo)
    if south == "flux":
        south_mirror(a, size, halo, interior)
    elif south is not None:
        south_vg(a, size, halo, *south, dy_row, interior)
    z_mirror(a, size, halo, bottom == "flux", top == "flux")
    z_vg(a, size, halo, _vg(bottom), _vg(top), dz)
    oracle.periodic_x_fill(a, size, halo)
    return a


def post_pass_sequence(oracle, a, xl, yl, sg, size, halo, south, bottom, top, dy_row, dz, horizontal=True):
    """The library's order: the whole horizontal fill, then the Value / Gradient south pass over whole padded rows, then the no-flux
    mirror of the Flux sides, then the Value / Gradient bottom / top pass (horizontal=False: skip the horizontal fill)"""
    if horizontal:
        oracle.fill_halo_regions(a, xl, yl, sg, size, halo)
    if _vg(south) is not None:
        south_vg(a, size, halo, *south, dy_row)
    if south == "flux":
        south_mirror(a, size, halo)
    z_mirror(a, size, halo, bottom == "flux", top == "flux")
    z_vg(a, size, halo, _vg(bottom), _vg(top), dz)
    return a


def periodic_rows(rng, rows, size, halo, dtype):
    """(rows, Nx+2Hx) array whose x halos are the periodic copy of its interior columns"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    inner = rng.uniform(0.5, 2.0, (rows, Nx)).astype(dtype)
    return np.concatenate([inner[:, Nx - Hx:], inner, inner[:, :Hx]], axis=1) if Hx else inner
