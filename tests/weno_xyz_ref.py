"""Host reference of the tracer tendency of `WENO()` -- WENO5 in x, y and z, walls in z -- in numpy, on padded parents: a statement of the
rule of include/tripolar_hip_weno_xyz.h written from the header's text.

[recalled: Oceananigans' WENO() = FluxFormAdvection(WENO(order = 5) x3) on a z-Bounded grid; parity unpinned, like every operator here]

Everything not named here is weno_ref's (the rule of include/tripolar_hip_weno.h), from which this module takes face_value (R5), the x and
y fluxes and the last line.  In the field type T, in exactly this order, every operation one correctly rounded IEEE operation:
    R3(q0, q1, q2):                       q1 is the upwind cell, q2 the downwind one
        p1 = T(1.5) * q1 - T(0.5) * q0
        p0 = T(0.5) * (q1 + q2)
        e1 = q1 - q0;  b1 = e1 * e1
        e0 = q2 - q1;  b0 = e0 * e0
        tau = |b0 - b1|
        r0 = tau / (b0 + eps);   r1 = tau / (b1 + eps)
        a0 = K(2,3) * (T(1) + r0 * r0);   a1 = K(1,3) * (T(1) + r1 * r1)
        R3 = (a0 * p0 + a1 * p1) / (a0 + a1)
    face f = 1 .. Nz+1 lies between levels f-1 and f;   dist(f) = min(f - 1, Nz + 1 - f)
        dist = 0:   C = T(0.5) * (c[f-1] + c[f])
        dist = 1:   C = Mz >= 0 ? c[f-1] : c[f]
        dist = 2:   C = Mz >= 0 ? R3(c[f-2], c[f-1], c[f]) : R3(c[f+1], c[f], c[f-1])
        dist >= 3:  C = Mz >= 0 ? R5(c[f-3], c[f-2], c[f-1], c[f], c[f+1]) : R5(c[f+2], c[f+1], c[f], c[f-1], c[f-2])
        Fz[i,j,f] = Mz[i,j,f] * C
`>= 0` is true for -0 and false for NaN; the inputs are selected, the face value is evaluated once per face.  A face with dist >= 1 reads
levels 1..Nz only; faces 1 and Nz + 1 read the planes 0 and Nz + 1.  So Hx >= 3, Hy >= 3, Hz >= 1.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1]; w's parent has Nz + 1 + 2 Hz planes."""
import numpy as np

import weno_ref
from weno_ref import face_value, same_bits, upwind_face_value  # noqa: F401  (re-exported)

CENTRED = 2                                                        # what face_order calls the centred mean of the two wall faces


def face_value3(q0, q1, q2):
    """R3(q0, q1, q2) on arrays of one floating dtype, operation for operation"""
    T = q0.dtype.type
    K = lambda n, d: T(n) / T(d)                                   # noqa: E731
    eps = T(1e-8)
    with np.errstate(all="ignore"):
        p1 = T(1.5) * q1 - T(0.5) * q0
        p0 = T(0.5) * (q1 + q2)
        e1 = q1 - q0
        b1 = e1 * e1
        e0 = q2 - q1
        b0 = e0 * e0
        tau = np.abs(b0 - b1)
        r0, r1 = tau / (b0 + eps), tau / (b1 + eps)
        a0, a1 = K(2, 3) * (T(1) + r0 * r0), K(1, 3) * (T(1) + r1 * r1)
        out = (a0 * p0 + a1 * p1) / (a0 + a1)
    assert out.dtype == q0.dtype
    return out


def face_order(f, Nz):
    """the order of the z-face f = 1 .. Nz + 1: 2 (the centred mean) at the two walls, 1 one face away, 3 two faces away, 5 from three on"""
    assert 1 <= f <= Nz + 1
    dist = min(f - 1, Nz + 1 - f)
    return (CENTRED, 1, 3)[dist] if dist < 3 else 5


def z_face_values(c, Mz, size, halo):
    """C at the Nz + 1 z-faces of the interior columns, (Nz + 1, Ny, Nx): Mz is (Nz + 1, Ny, Nx), c a padded parent"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    T = c.dtype.type
    col = c[:, Hy:Hy + Ny, Hx:Hx + Nx]
    level = lambda n: col[Hz + n - 1]                             # noqa: E731  level n = 0 .. Nz + 1 (1-based; 0 and Nz + 1 the halo planes)
    out = np.empty((Nz + 1, Ny, Nx), c.dtype)
    with np.errstate(all="ignore"):
        for f in range(1, Nz + 2):
            order, pos = face_order(f, Nz), Mz[f - 1] >= 0         # True for -0, False for NaN
            if order == CENTRED:
                C = T(0.5) * (level(f - 1) + level(f))
            elif order == 1:
                C = np.where(pos, level(f - 1), level(f))
            elif order == 3:
                C = face_value3(np.where(pos, level(f - 2), level(f + 1)), np.where(pos, level(f - 1), level(f)),
                                np.where(pos, level(f), level(f - 1)))
            else:
                x = [level(f + o) for o in range(-3, 3)]
                C = face_value(*(np.where(pos, x[n], x[5 - n]) for n in range(5)))
            out[f - 1] = C
    return out


def fluxes(c, u, v, w, dy_fc, dx_cf, az_cc, dz_c, size, halo):
    """(Fx, Fy, Fz, V) of the rule: Fx (Nz, Ny, Nx + 1), Fy (Nz, Ny + 1, Nx), Fz (Nz + 1, Ny, Nx), V (Nz, Ny, Nx)"""
    T = c.dtype
    assert all(a.dtype == T for a in (u, v, w, dy_fc, dx_cf, az_cc, dz_c))
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert Hx >= 3 and Hy >= 3 and Hz >= 1 and dz_c.shape == (Nz,) and c.shape == u.shape == v.shape == (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    assert w.shape == (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    ys, xs, zs = slice(Hy, Hy + Ny), slice(Hx, Hx + Nx), slice(Hz, Hz + Nz)
    with np.errstate(all="ignore"):
        d = dz_c[:, None, None]
        Mx = (dy_fc[None, ys, Hx:Hx + Nx + 1] * d) * u[zs, ys, Hx:Hx + Nx + 1]
        My = (dx_cf[None, Hy:Hy + Ny + 1, xs] * d) * v[zs, Hy:Hy + Ny + 1, xs]
        Mz = az_cc[None, ys, xs] * w[Hz:Hz + Nz + 1, ys, xs]
        Fx = Mx * upwind_face_value(Mx, [c[zs, ys, Hx + o:Hx + o + Nx + 1] for o in range(-3, 3)])
        Fy = My * upwind_face_value(My, [c[zs, Hy + o:Hy + o + Ny + 1, xs] for o in range(-3, 3)])
        Fz = Mz * z_face_values(c, Mz, size, halo)
        V = az_cc[None, ys, xs] * d
    return Fx, Fy, Fz, V


def interior_tendency(c, u, v, w, dy_fc, dx_cf, az_cc, dz_c, size, halo):
    """G on the interior, (Nz, Ny, Nx), in the dtype of c, unmasked"""
    (Nx, Ny, Nz) = size
    Fx, Fy, Fz, V = fluxes(c, u, v, w, dy_fc, dx_cf, az_cc, dz_c, size, halo)
    one = c.dtype.type(1)
    with np.errstate(all="ignore"):
        G = -((one / V) * (((Fx[:, :, 1:] - Fx[:, :, :-1]) + (Fy[:, 1:, :] - Fy[:, :-1, :])) + (Fz[1:] - Fz[:-1])))
    assert G.dtype == c.dtype and G.shape == (Nz, Ny, Nx)
    return G


def tendency(c, u, v, w, G0, dy_fc, dx_cf, az_cc, dz_c, size, halo, n_cc=None, mask_value=0.0):
    """the parent of G after the call: a copy of `G0` with the interior replaced, halo cells untouched"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    G = interior_tendency(c, u, v, w, dy_fc, dx_cf, az_cc, dz_c, size, halo)
    if n_cc is not None:
        assert n_cc.shape == (Ny, Nx)
        k = np.arange(1, Nz + 1)[:, None, None]
        G = np.where(k <= np.minimum(np.maximum(n_cc.astype(np.int64), 0), Nz)[None], c.dtype.type(mask_value), G)
    assert G0.shape == c.shape
    out = G0.copy()
    out[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = G
    return out


def cells_read(size, halo):
    """boolean masks of the cells the rule reads, as weno_ref.cells_read gives them, with the z-arm of c written from the order table: the
    interior columns at the planes 0 .. Nz + 1 (both wall faces read their halo plane, every other face levels 1 .. Nz only)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    read = weno_ref.cells_read(size, halo)
    planes = np.zeros(Nz + 2 * Hz, bool)                           # the planes of the interior columns that some z-face reads
    for f in range(1, Nz + 2):
        order = face_order(f, Nz)
        lo, hi = {CENTRED: (f - 1, f), 1: (f - 1, f), 3: (f - 2, f + 1), 5: (f - 3, f + 2)}[order]
        assert order == CENTRED or (lo >= 1 and hi <= Nz)
        planes[Hz + lo - 1:Hz + hi] = True
    read["c"][:, Hy:Hy + Ny, Hx:Hx + Nx] = planes[:, None, None]   # every level is its own x- and y-face's cell too, and lies in 1 .. Nz
    return read


def dependence_window(level, size, positive):
    """The levels k = 1 .. Nz of G that may change when c changes at `level` (1 .. Nz) of a column and w has one sign everywhere, u and v
    being zero: face f reads, by its order and the sign, the levels listed in the header; node k reads its faces k and k + 1.  Returns a
    boolean (Nz,), index k - 1."""
    Nz = size[2]
    reads = np.zeros(Nz + 2, bool)                                 # per face f (index f), whether it reads `level`
    for f in range(1, Nz + 2):
        order = face_order(f, Nz)
        if order == CENTRED:
            cells = (f - 1, f)
        elif order == 1:
            cells = (f - 1,) if positive else (f,)
        elif order == 3:
            cells = (f - 2, f - 1, f) if positive else (f + 1, f, f - 1)
        else:
            cells = tuple(range(f - 3, f + 2)) if positive else tuple(range(f - 2, f + 3))
        reads[f] = level in cells
    return np.array([reads[k] or reads[k + 1] for k in range(1, Nz + 1)])
