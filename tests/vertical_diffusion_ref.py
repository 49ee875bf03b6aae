"""The rule of tpg_vertical_implicit_diffusion (include/tripolar_hip_vertical_diffusion.h) in numpy, in the field type, level by level: the
reference the GPU tests compare with bit for bit, itself held to properties by tests/test_vertical_diffusion_ref.py.

Two statements of the one rule: solve_column, the header's lines word for word on one column with 1-based arrays and Python scalars of the
field type, and solve_columns, the same operations on whole planes at once (what the GPU tests can afford); the property tests require the
two to agree bit for bit.  Neither uses a fused operation: numpy's scalar and array arithmetic rounds every operation once."""
import numpy as np

CONSTANT, PROFILE, FIELD = 0, 1, 2


def first_wet(count, Nz):
    """k0 of the header, 1-based: the first cell of the column that is solved"""
    return 1 if count is None else min(max(int(count), 0), Nz) + 1


def solve_column(f, kappa, dz_c, dz_f, dt, count=None, mask_value=0.0):
    """One column.  f: Nz values; kappa, dz_f: Nz + 1 values at the faces 1..Nz+1; dz_c: Nz values; all of one floating type.  Returns phi.
    Entries the rule does not read are not touched (they may hold anything)."""
    T = f.dtype.type
    Nz = len(f)
    F = lambda a: [None] + [T(x) for x in a]                      # noqa: E731    1-based
    f1, kap, dzc, dzf = F(f), F(kappa), F(dz_c), F(dz_f)
    k0 = first_wet(count, Nz)
    dtT, one = T(dt), T(1)
    small = T(10) * np.finfo(T).eps
    phi = [None] + [T(mask_value)] * Nz
    if k0 > Nz:
        return np.array(phi[1:], dtype=T)
    up, lo, t = {}, {}, {}
    with np.errstate(all="ignore"):
        for k in range(k0 + 1, Nz + 1):
            up[k - 1] = -(dtT * ((kap[k] / dzc[k - 1]) / dzf[k]))
            lo[k] = -(dtT * ((kap[k] / dzc[k]) / dzf[k]))

        def diag(k):
            d = one
            if k in up:
                d = d - up[k]
            if k in lo:
                d = d - lo[k]
            return d
        beta = diag(k0)
        phi[k0] = f1[k0] / beta
        for k in range(k0 + 1, Nz + 1):
            t[k] = up[k - 1] / beta
            beta = diag(k) - lo[k] * t[k]
            phi[k] = (f1[k] - lo[k] * phi[k - 1]) / beta if abs(beta) > small else f1[k]
        for k in range(Nz - 1, k0 - 1, -1):
            phi[k] = phi[k] - t[k + 1] * phi[k + 1]
    return np.array(phi[1:], dtype=T)


def solve_columns(f, kappa, dz_c, dz_f, dt, counts=None, mask_value=0.0):
    """Many columns at once.  f: (Nz, ...) of a floating type T; kappa: (Nz + 1,) or (Nz + 1, ...) values at the faces (0-based: face k lies
    under cell k; the faces 0 and Nz are never used); dz_c: Nz, dz_f: Nz + 1 values; counts: None or an integer array of f's column shape.
    Returns phi, of f's shape and type."""
    T = f.dtype.type
    Nz, shape = f.shape[0], f.shape[1:]
    kap = np.asarray(kappa, dtype=T)
    kap = kap.reshape(kap.shape + (1,) * (1 + len(shape) - kap.ndim))
    dz_c, dz_f = np.asarray(dz_c, dtype=T), np.asarray(dz_f, dtype=T)
    m = np.zeros(shape, dtype=np.int64) if counts is None else np.clip(np.asarray(counts, dtype=np.int64), 0, Nz)
    dtT, one, zero, mval = T(dt), T(1), T(0), T(mask_value)
    small = T(10) * np.finfo(T).eps
    phi, t = np.empty_like(f), np.zeros_like(f)
    beta, up_below = np.full(shape, one, dtype=T), np.zeros(shape, dtype=T)
    with np.errstate(all="ignore"):
        for k in range(Nz):
            open_lo, open_up = k > m, k + 1 < Nz
            up = np.broadcast_to(-(dtT * ((kap[k + 1] / dz_c[k]) / dz_f[k + 1])), shape) if open_up else np.zeros(shape, dtype=T)
            lo = np.broadcast_to(-(dtT * ((kap[k] / dz_c[k]) / dz_f[k])), shape) if k > 0 else np.zeros(shape, dtype=T)
            diag = np.where(open_lo, (one - up) - lo if open_up else one - lo, one - up if open_up else np.full(shape, one, dtype=T))
            t[k] = np.where(open_lo, up_below / beta, zero)
            beta = np.where(open_lo, diag - lo * t[k], diag)
            below = phi[k - 1] if k > 0 else f[k]
            num = np.where(open_lo, f[k] - lo * below, f[k])
            elide = open_lo & ~(np.abs(beta) > small)
            phi[k] = np.where(k < m, mval, np.where(elide, f[k], num / beta))
            up_below = up
        for k in range(Nz - 2, -1, -1):
            phi[k] = np.where(k >= m, phi[k] - t[k + 1] * phi[k + 1], phi[k])
    assert phi.dtype == f.dtype
    return phi


def face_values(kappa, form, size, halo, dtype):
    """the (Nz + 1, ...) face array solve_columns takes, from the `kappa` of a call in the form `form`: a number, Nz + 1 values, or a padded
    parent whose face k (0-based) is the plane Hz + k.  The faces 0 and Nz hold NaN: the rule never uses them"""
    Nx, Ny, Nz = size
    Hx, Hy, Hz = halo
    if form == CONSTANT:
        return np.full(Nz + 1, dtype(kappa), dtype=dtype)
    if form == PROFILE:
        return np.asarray(kappa, dtype=dtype).copy()
    out = np.full((Nz + 1, Ny, Nx), np.nan, dtype=dtype)
    out[1:Nz] = kappa[Hz + 1:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    return out


def reference(parents, kappa, form, dz_c, dz_f, dt, size, halo, counts=None, mask_value=0.0):
    """what the call leaves in the padded parents `parents` (a list of (Nz + 2Hz, Ny + 2Hy, Nx + 2Hx) arrays): new arrays, the halos as
    they were"""
    Nx, Ny, Nz = size
    Hx, Hy, Hz = halo
    kap = face_values(kappa, form, size, halo, parents[0].dtype.type)
    out = []
    for parent in parents:
        new = parent.copy()
        new[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = solve_columns(parent[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], kap, dz_c, dz_f, dt, counts, mask_value)
        out.append(new)
    return out
