"""Host reference of the WENO5 flux-form advection tendency of a tracer in numpy, on padded parents: a statement of the rule of
include/tripolar_hip_weno.h written from the header's text.

[recalled: Oceananigans' FluxFormAdvection(WENO(order = 5), WENO(order = 5), Centered()), uniform-grid coefficients, Jiang-Shu smoothness
indicators, WENO-Z weights, eps = 1e-8; parity unpinned, like every operator here]

The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz, in the field type T, in exactly this order, with no contraction; every
operation is one correctly rounded IEEE operation.
    K(n, d) = T(n) / T(d);  eps = T(1e-8);  S(a, b, c) = (a - T(2) * b) + c
    R(q0, q1, q2, q3, q4):                     q2 is the upwind cell, q3 the downwind one
        p2 = (K(1,3) * q0 - K(7,6) * q1) + K(11,6) * q2
        p1 = (K(5,6) * q2 - K(1,6) * q1) + K(1,3)  * q3
        p0 = (K(1,3) * q2 + K(5,6) * q3) - K(1,6)  * q4
        s2 = S(q0,q1,q2);  d2 = (q0 - T(4) * q1) + T(3) * q2;          b2 = K(13,12) * (s2 * s2) + T(0.25) * (d2 * d2)
        s1 = S(q1,q2,q3);  d1 = q1 - q3;                                b1 = K(13,12) * (s1 * s1) + T(0.25) * (d1 * d1)
        s0 = S(q2,q3,q4);  d0 = (T(3) * q2 - T(4) * q3) + q4;           b0 = K(13,12) * (s0 * s0) + T(0.25) * (d0 * d0)
        tau = |b0 - b2|
        r0 = tau / (b0 + eps);   r1 = tau / (b1 + eps);   r2 = tau / (b2 + eps)
        a0 = K(3,10) * (T(1) + r0 * r0);   a1 = K(3,5) * (T(1) + r1 * r1);   a2 = K(1,10) * (T(1) + r2 * r2)
        R  = ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2)
    Fx[i,j,k] = Mx[i,j,k] * ( Mx[i,j,k] >= 0 ? R(c[i-3], c[i-2], c[i-1], c[i], c[i+1]) : R(c[i+2], c[i+1], c[i], c[i-1], c[i-2]) )
    Fy[i,j,k] = My[i,j,k] * ( My[i,j,k] >= 0 ? R(c[j-3], c[j-2], c[j-1], c[j], c[j+1]) : R(c[j+2], c[j+1], c[j], c[j-1], c[j-2]) )
    Fz[i,j,k] = Mz[i,j,k] * (T(0.5) * (c[i,j,k-1] + c[i,j,k]))
    G[i,j,k]  = -((T(1) / V) * (((Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])) + (Fz[i,j,k+1] - Fz[i,j,k])))
with Mx, My, Mz, V as in advection_ref.  `>= 0` is true for -0 and false for NaN.  Cells read: c[-2..Nx+3, j, k], c[i, -2..Ny+3, k],
c[i, j, 0..Nz+1]; u, v, w and the metrics as in advection_ref.  So Hx >= 3, Hy >= 3, Hz >= 1.  Only interior cells of G are written; the
mask is advection_ref's.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1]; w's parent has Nz + 1 + 2 Hz planes.  numpy's elementwise arithmetic in a dtype is
one correctly rounded IEEE operation per operation: the reference is exact, comparisons are bit for bit."""
import numpy as np

from vorticity_ref import same_bits  # noqa: F401  (re-exported: the comparison every test of this operator uses)

# the stencil, derived from the rule above: (array, di, dj, dk) of every cell a node (i, j, k) reads
STENCIL = (tuple(("c", di, 0, 0) for di in range(-3, 4)) + tuple(("c", 0, dj, 0) for dj in range(-3, 4) if dj)
           + (("c", 0, 0, -1), ("c", 0, 0, 1),
              ("u", 0, 0, 0), ("u", 1, 0, 0), ("dy_fc", 0, 0, 0), ("dy_fc", 1, 0, 0),
              ("v", 0, 0, 0), ("v", 0, 1, 0), ("dx_cf", 0, 0, 0), ("dx_cf", 0, 1, 0),
              ("w", 0, 0, 0), ("w", 0, 0, 1), ("az_cc", 0, 0, 0)))


def face_value(q0, q1, q2, q3, q4):
    """R(q0, q1, q2, q3, q4) on arrays of one floating dtype, operation for operation"""
    T = q0.dtype.type
    K = lambda n, d: T(n) / T(d)                                   # noqa: E731
    eps = T(1e-8)
    S = lambda a, b, c: (a - T(2) * b) + c                         # noqa: E731
    with np.errstate(all="ignore"):
        p2 = (K(1, 3) * q0 - K(7, 6) * q1) + K(11, 6) * q2
        p1 = (K(5, 6) * q2 - K(1, 6) * q1) + K(1, 3) * q3
        p0 = (K(1, 3) * q2 + K(5, 6) * q3) - K(1, 6) * q4
        s2, d2 = S(q0, q1, q2), (q0 - T(4) * q1) + T(3) * q2
        s1, d1 = S(q1, q2, q3), q1 - q3
        s0, d0 = S(q2, q3, q4), (T(3) * q2 - T(4) * q3) + q4
        b2 = K(13, 12) * (s2 * s2) + T(0.25) * (d2 * d2)
        b1 = K(13, 12) * (s1 * s1) + T(0.25) * (d1 * d1)
        b0 = K(13, 12) * (s0 * s0) + T(0.25) * (d0 * d0)
        tau = np.abs(b0 - b2)
        r0, r1, r2 = tau / (b0 + eps), tau / (b1 + eps), tau / (b2 + eps)
        a0, a1, a2 = K(3, 10) * (T(1) + r0 * r0), K(3, 5) * (T(1) + r1 * r1), K(1, 10) * (T(1) + r2 * r2)
        out = ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2)
    assert out.dtype == q0.dtype
    return out


def upwind_face_value(M, x):
    """M >= 0 ? R(x[0], x[1], x[2], x[3], x[4]) : R(x[5], x[4], x[3], x[2], x[1]) for the six cells x[0..5] around the face between x[2]
    and x[3]: the five inputs are selected, R is evaluated once"""
    pos = M >= 0                                                   # True for -0, False for NaN
    return face_value(*(np.where(pos, x[n], x[5 - n]) for n in range(5)))


def interior_tendency(c, u, v, w, dy_fc, dx_cf, az_cc, dz_c, size, halo):
    """G on the interior, (Nz, Ny, Nx), in the dtype of c, unmasked"""
    T = c.dtype
    assert all(a.dtype == T for a in (u, v, w, dy_fc, dx_cf, az_cc, dz_c))
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert Hx >= 3 and Hy >= 3 and Hz >= 1 and dz_c.shape == (Nz,) and c.shape == u.shape == v.shape == (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    assert w.shape == (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    half, one = T.type(0.5), T.type(1)
    ys, xs, zs = slice(Hy, Hy + Ny), slice(Hx, Hx + Nx), slice(Hz, Hz + Nz)
    with np.errstate(all="ignore"):
        d = dz_c[:, None, None]
        Mx = (dy_fc[None, ys, Hx:Hx + Nx + 1] * d) * u[zs, ys, Hx:Hx + Nx + 1]
        My = (dx_cf[None, Hy:Hy + Ny + 1, xs] * d) * v[zs, Hy:Hy + Ny + 1, xs]
        Mz = az_cc[None, ys, xs] * w[Hz:Hz + Nz + 1, ys, xs]
        # the six cells i-3 .. i+2 around each of the Nx + 1 x-faces, j-3 .. j+2 around each of the Ny + 1 y-faces
        Fx = Mx * upwind_face_value(Mx, [c[zs, ys, Hx + o:Hx + o + Nx + 1] for o in range(-3, 3)])
        Fy = My * upwind_face_value(My, [c[zs, Hy + o:Hy + o + Ny + 1, xs] for o in range(-3, 3)])
        Fz = Mz * (half * (c[Hz - 1:Hz + Nz, ys, xs] + c[Hz:Hz + Nz + 1, ys, xs]))
        V = az_cc[None, ys, xs] * d
        G = -((one / V) * (((Fx[:, :, 1:] - Fx[:, :, :-1]) + (Fy[:, 1:, :] - Fy[:, :-1, :])) + (Fz[1:] - Fz[:-1])))
    assert G.dtype == T and G.shape == (Nz, Ny, Nx)
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
    """boolean masks of the cells the rule reads, derived from STENCIL: {"c", "u", "v": parent-shaped; "w": its own longer parent; "dy_fc",
    "dx_cf", "az_cc": plane-shaped}"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    plane, parent = (Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    read = {"c": np.zeros(parent, bool), "u": np.zeros(parent, bool), "v": np.zeros(parent, bool),
            "w": np.zeros((Nz + 1 + 2 * Hz,) + plane, bool),
            "dy_fc": np.zeros(plane, bool), "dx_cf": np.zeros(plane, bool), "az_cc": np.zeros(plane, bool)}
    for name, di, dj, dk in STENCIL:
        ys, xs = slice(Hy + dj, Hy + dj + Ny), slice(Hx + di, Hx + di + Nx)
        p = read[name]
        (p[ys, xs] if p.ndim == 2 else p[Hz + dk:Hz + dk + Nz, ys, xs])[...] = True
    return read


def dependence_window(changed, size, halo, axis, positive):
    """The interior nodes of G that may change when the cells `changed` (a boolean parent of c, halos included) change and the flow along
    `axis` ("x" with u, "y" with v) has one sign everywhere, the other two velocities being zero: a face's value reads the cells
    f-3 .. f+1 (flow >= 0) or f-2 .. f+2 (flow < 0) along the axis, and a node its two faces n and n+1 -- so a changed cell n* reaches the
    nodes n*-2 .. n*+3 or n*-3 .. n*+2 of its row (column) and level, no others.  Returns a boolean (Nz, Ny, Nx)."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    lo, hi = (-2, 3) if positive else (-3, 2)
    reach = np.zeros(changed.shape, bool)
    ax = 2 if axis == "x" else 1
    n = changed.shape[ax]
    for o in range(lo, hi + 1):                                    # node = cell + o
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        src[ax] = slice(max(0, -o), n - max(0, o))
        dst[ax] = slice(max(0, o), n - max(0, -o))
        reach[tuple(dst)] |= changed[tuple(src)]
    return reach[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
