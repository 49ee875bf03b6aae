"""Host reference of the barotropic mode and the split-explicit velocity correction in numpy, on padded parents.

The rule [recalled: Oceananigans' `compute_barotropic_mode!` and `barotropic_split_explicit_corrector!`; parity unpinned, like every operator
here.]

Arrays
- `u` at (Face, Center, Center) and `v` at (Center, Face, Center): padded parents of geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
- `U`, `V`, `Ubar`, `Vbar`: 2-D padded planes of `(Ny + 2 Hy2) x (Nx + 2 Hx)`: the same `Hx` as the 3-D fields, their own north / south halo
  `Hy2`.
- `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]`; `depth_of_count`: `Nz + 1` values, `depth_of_count[n]` the depth of a column whose lowest `n` cells are immersed.
The mode, for every interior column `i = 1..Nx`, `j = 1..Ny`, in the field type, in exactly this order, every operation one correctly rounded
IEEE operation:
    Ubar[i,j] = dz_c[1] * u[i,j,1]
    for k = 2..Nz:  Ubar[i,j] = Ubar[i,j] + dz_c[k] * u[i,j,k]
and Vbar from v likewise.  The correction, in place, for every interior node:
    H = depth_of_count[min(n_fc[i,j], Nz)]        (n_fc None: depth_of_count[0])
    c = (U[i,j] - Ubar[i,j]) / H                  one subtraction, one division, formed once per column
    u[i,j,k] = u[i,j,k] + c      k = 1..Nz
and v likewise with V, Vbar, n_cf.  Where a count plane is given, nodes k <= n hold the mask value instead (what tpg_mask_immersed_fields
leaves on a z-Center field).  No halo cell of any array is read; only interior cells are written.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1], 2-D planes [j + Hy2 - 1, i + Hx - 1].  numpy's elementwise arithmetic in the dtype is
one correctly rounded IEEE operation per operation: the reference is exact, comparisons are bit for bit."""
import numpy as np

from vorticity_ref import same_bits  # noqa: F401  (re-exported: the comparison every test of these passes uses)


def _in3(p, size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return p[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]


def _in2(p, size, halo, Hy2):
    (Nx, Ny, _), (Hx, _, _) = size, halo
    assert p.shape == (Ny + 2 * Hy2, Nx + 2 * Hx), (p.shape, size, halo, Hy2)
    return p[Hy2:Hy2 + Ny, Hx:Hx + Nx]


def interior_mode(f, dz_c, size, halo):
    """Σ_k dz_c[k] f[., ., k] in the fixed order k = 1..Nz on the interior: (Ny, Nx) in the dtype of f"""
    T = f.dtype
    assert dz_c.dtype == T and dz_c.shape == (size[2],)
    x = _in3(f, size, halo)
    with np.errstate(all="ignore"):
        acc = dz_c[0] * x[0]
        for k in range(1, size[2]):
            acc = acc + dz_c[k] * x[k]
    assert acc.dtype == T
    return acc


def barotropic_mode(u, v, Ubar0, Vbar0, dz_c, size, halo, Hy2):
    """the planes (Ubar, Vbar) after the call: copies of `Ubar0`, `Vbar0` with the interior replaced, halo cells untouched.  A pair (u, Ubar0)
    or (v, Vbar0) may be None -> None."""
    out = []
    for f, p0 in ((u, Ubar0), (v, Vbar0)):
        assert (f is None) == (p0 is None)
        if f is None:
            out.append(None)
            continue
        p = p0.copy()
        _in2(p, size, halo, Hy2)[...] = interior_mode(f, dz_c, size, halo)
        out.append(p)
    return tuple(out)


def interior_correction(f, t, tbar, depth_of_count, size, halo, Hy2, n=None, mask_value=0.0):
    """the corrected interior (Nz, Ny, Nx) of the parent f"""
    T = f.dtype
    Nz = size[2]
    assert t.dtype == T and tbar.dtype == T and depth_of_count.dtype == T and depth_of_count.shape == (Nz + 1,)
    idx = np.zeros((size[1], size[0]), np.int64) if n is None else np.minimum(n.astype(np.int64), Nz)
    with np.errstate(all="ignore"):
        c = (_in2(t, size, halo, Hy2) - _in2(tbar, size, halo, Hy2)) / depth_of_count[idx]
        out = _in3(f, size, halo) + c[None]
    if n is not None:
        out = np.where(np.arange(1, Nz + 1)[:, None, None] <= n[None], T.type(mask_value), out)
    assert out.dtype == T
    return out


def barotropic_correction(u, v, U, V, Ubar, Vbar, depth_of_count, size, halo, Hy2, n_fc=None, n_cf=None, mask_value=0.0):
    """the parents (u, v) after the call: copies with the interior replaced, halo cells untouched.  A triple (u, U, Ubar) or (v, V, Vbar) may be
    None -> None."""
    out = []
    for f, t, tb, n in ((u, U, Ubar, n_fc), (v, V, Vbar, n_cf)):
        assert (f is None) == (t is None) == (tb is None)
        if f is None:
            out.append(None)
            continue
        p = f.copy()
        _in3(p, size, halo)[...] = interior_correction(f, t, tb, depth_of_count, size, halo, Hy2, n, mask_value)
        out.append(p)
    return tuple(out)


def cells_read(size, halo, Hy2, n_fc=None, n_cf=None):
    """boolean masks of the cells the rules read: {"field": parent-shaped (u and v alike: the interior), "plane": 2-D-plane-shaped (U, V, Ubar,
    Vbar alike: the interior), "depth_of_count": the Nz + 1 entries some count selects (entry 0 alone without a plane)}"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    field = np.zeros((Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), bool)
    _in3(field, size, halo)[...] = True
    plane = np.zeros((Ny + 2 * Hy2, Nx + 2 * Hx), bool)
    _in2(plane, size, halo, Hy2)[...] = True
    depth = np.zeros(Nz + 1, bool)
    for n in (n_fc, n_cf):
        if n is None:
            depth[0] = True
        else:
            depth[np.minimum(n.astype(np.int64), Nz)] = True
    return {"field": field, "plane": plane, "depth_of_count": depth}
