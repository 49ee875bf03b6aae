"""Host reference of the quasi-Adams-Bashforth-2 step of the velocities and tracers and of the barotropic forcing, in numpy, on padded parents.

The rule [recalled: Oceananigans' QuasiAdamsBashforth2 `ab2_step_velocities!`, `ab2_step_tracers!`, `store_tendencies!` and, for a
split-explicit free surface, `_compute_integrated_ab2_tendencies!`; parity unpinned, like every operator here.]

Arrays
- the field `x` (u, v, a tracer) and its tendencies `Gn` (this step's), `Gm` (the previous step's): padded parents of one geometry
  `(Nx, Ny, Nz, Hx, Hy, Hz)`.
- `G` (GU, GV): a 2-D padded plane of `(Ny + 2 Hy2) x (Nx + 2 Hx)`: the same `Hx` as the 3-D fields, its own north / south halo `Hy2`.
- `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]`; `n`: None, or a count plane (Ny, Nx) of int32.
For every interior node, in the field type T, in exactly this order, every operation one correctly rounded IEEE operation:
    c1 = T(1.5) + T(chi)         c2 = T(0.5) + T(chi)
    g  = c1 * Gn[i,j,k] - c2 * Gm[i,j,k]          euler:  g = c1 * Gn[i,j,k], Gm is NOT read
    x[i,j,k] = x[i,j,k] + T(dt) * g
    store:  Gm[i,j,k] = Gn[i,j,k]
    ĝ_k = +0 where k <= min(max(n[i,j], 0), Nz), g otherwise
    G[i,j] = dz_c[1] * ĝ_1;     for k = 2..Nz:  G[i,j] = G[i,j] + dz_c[k] * ĝ_k
No halo cell of any array is read; only interior cells are written.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1], 2-D planes [j + Hy2 - 1, i + Hx - 1].  numpy's elementwise arithmetic in the dtype is
one correctly rounded IEEE operation per operation, level by level: the reference is exact, comparisons are bit for bit."""
import numpy as np

from vorticity_ref import same_bits  # noqa: F401  (re-exported: the comparison every test of these passes uses)

EULER, STORE = 1, 2                                                # the flag bits of include/tripolar_hip_timestep.h


def _in3(p, size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return p[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]


def _in2(p, size, halo, Hy2):
    (Nx, Ny, _), (Hx, _, _) = size, halo
    assert p.shape == (Ny + 2 * Hy2, Nx + 2 * Hx), (p.shape, size, halo, Hy2)
    return p[Hy2:Hy2 + Ny, Hx:Hx + Nx]


def constants(dt, chi, T):
    """(c1, c2, dt) in the type T: one addition each, the conversions of chi and dt once"""
    T = np.dtype(T).type
    chi_t = T(chi)
    return T(1.5) + chi_t, T(0.5) + chi_t, T(dt)


def interior_step(x, Gn, Gm, dt, chi, flags, size, halo, dz_c=None, n=None):
    """(the stepped interior (Nz, Ny, Nx) of x, the interior integral (Ny, Nx) or None without dz_c), level by level"""
    T = x.dtype
    Nz = size[2]
    euler = bool(flags & EULER)
    assert Gn.dtype == T and (euler or Gm.dtype == T) and (dz_c is None or (dz_c.dtype == T and dz_c.shape == (Nz,)))
    c1, c2, dt_t = constants(dt, chi, T)
    xs, gn = _in3(x, size, halo), _in3(Gn, size, halo)
    gm = None if euler else _in3(Gm, size, halo)
    m = None if n is None else np.minimum(np.maximum(n.astype(np.int64), 0), Nz)
    out = np.empty(xs.shape, T)
    acc = None
    with np.errstate(all="ignore"):
        for k in range(Nz):
            if euler:
                g = c1 * gn[k]
            else:
                g = c1 * gn[k] - c2 * gm[k]
            out[k] = xs[k] + dt_t * g
            if dz_c is not None:
                gh = g if m is None else np.where(k + 1 <= m, T.type(0), g)
                acc = dz_c[k] * gh if k == 0 else acc + dz_c[k] * gh
            assert g.dtype == T
    assert out.dtype == T and (acc is None or acc.dtype == T)
    return out, acc


def ab2_step(x, Gn, Gm, dt, chi, flags, size, halo, G0=None, dz_c=None, Hy2=0, n=None):
    """the arrays (x, Gm, G) after the call on one field: copies with the interior replaced, halo cells untouched; Gm as it was without STORE
    (None stays None), G None without G0"""
    step, integral = interior_step(x, Gn, Gm, dt, chi, flags, size, halo, dz_c if G0 is not None else None, n)
    out = x.copy()
    _in3(out, size, halo)[...] = step
    prev = None if Gm is None else Gm.copy()
    if flags & STORE:
        _in3(prev, size, halo)[...] = _in3(Gn, size, halo)
    G = None
    if G0 is not None:
        G = G0.copy()
        _in2(G, size, halo, Hy2)[...] = integral
    return out, prev, G


def cells_read(size, halo, Hy2=0):
    """boolean masks of the cells the rule reads: {"field": parent-shaped (x, Gn, and Gm without EULER: the interior), "plane": nothing of a
    2-D plane is read (all False)}"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    field = np.zeros((Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), bool)
    _in3(field, size, halo)[...] = True
    return {"field": field, "plane": np.zeros((Ny + 2 * Hy2, Nx + 2 * Hx), bool)}
