"""Host reference of the vector-invariant advection tendency of the horizontal velocities of the drivers' scheme,
WENOVectorInvariant(vorticity_order = 5), in numpy, on padded parents: a statement of the rule of include/tripolar_hip_weno_vs.h written
from the header's text.

[recalled: Oceananigans' biased WENO weights for VelocityStencil -- the smoothness indicators of the tangential stencils of u averaged in y
and v averaged in x onto (Face, Face), summed and halved (beta_sum); parity unpinned, like every operator here]

Taken from the existing references, the one statement of each: vu, bu, vv (vvert), bv (weno_vi_ref.terms); Z and vhat, uhat
(weno_momentum_ref.zeta_at, transverse).  New here, in the field type T, in exactly this order:
    UB[i,j,k] = T(0.5) * (u[i,j-1,k] + u[i,j,k])        VB[i,j,k] = T(0.5) * (v[i-1,j,k] + v[i,j,k])
    W5V(q0..q4; a0..a4; b0..b4) = R(q0..q4) with b_s = T(0.5) * (bA_s + bB_s), bA_s the indicator of a0..a4, bB_s that of b0..b4
 u: zr = vhat >= 0 ? W5V(Z[i, j-2..j+2]; UB[i, j-2..j+2]; VB[i, j-2..j+2]) : W5V(Z[i, j+3..j-1]; UB[i, j+3..j-1]; VB[i, j+3..j-1])
    hu = -(vhat * zr);   Gu = -((hu + vu) + bu)
 v: zr = uhat >= 0 ? W5V(Z[i-2..i+2, j]; UB[i-2..i+2, j]; VB[i-2..i+2, j]) : W5V(Z[i+3..i-1, j]; UB[i+3..i-1, j]; VB[i+3..i-1, j])
    hv = uhat * zr;      Gv = -((hv + vvert) + bv)
`>= 0` is true for -0 and false for NaN: the fifteen inputs are selected, W5V is evaluated once.  Hx, Hy >= 3, Hz >= 1.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1].  numpy's elementwise arithmetic in a dtype is one correctly rounded IEEE operation
per operation: the reference is exact, comparisons are bit for bit."""
import numpy as np

import weno_momentum_ref
import weno_vi_ref
from momentum_ref import METRICS, _win, same_bits  # noqa: F401  (same_bits re-exported: the comparison every test of this operator uses)
from weno_vi_ref import cells_read  # noqa: F401  (the rule reads no cell weno_vi's does not read: the one statement)


def face_value_vs(q, a, b):
    """W5V(q[0..4]; a[0..4]; b[0..4]) on arrays of one floating dtype, operation for operation"""
    q0, q1, q2, q3, q4 = q
    T = q0.dtype.type
    K = lambda n, d: T(n) / T(d)                                   # noqa: E731
    eps = T(1e-8)

    def indicators(t0, t1, t2, t3, t4):
        s2, d2 = (t0 - T(2) * t1) + t2, (t0 - T(4) * t1) + T(3) * t2
        s1, d1 = (t1 - T(2) * t2) + t3, t1 - t3
        s0, d0 = (t2 - T(2) * t3) + t4, (T(3) * t2 - T(4) * t3) + t4
        return (K(13, 12) * (s2 * s2) + T(0.25) * (d2 * d2), K(13, 12) * (s1 * s1) + T(0.25) * (d1 * d1),
                K(13, 12) * (s0 * s0) + T(0.25) * (d0 * d0))

    with np.errstate(all="ignore"):
        p2 = (K(1, 3) * q0 - K(7, 6) * q1) + K(11, 6) * q2
        p1 = (K(5, 6) * q2 - K(1, 6) * q1) + K(1, 3) * q3
        p0 = (K(1, 3) * q2 + K(5, 6) * q3) - K(1, 6) * q4
        (bA2, bA1, bA0), (bB2, bB1, bB0) = indicators(*a), indicators(*b)
        b2, b1, b0 = T(0.5) * (bA2 + bB2), T(0.5) * (bA1 + bB1), T(0.5) * (bA0 + bB0)
        tau = np.abs(b0 - b2)
        r0, r1, r2 = tau / (b0 + eps), tau / (b1 + eps), tau / (b2 + eps)
        a0, a1, a2 = K(3, 10) * (T(1) + r0 * r0), K(3, 5) * (T(1) + r1 * r1), K(1, 10) * (T(1) + r2 * r2)
        out = ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2)
    out = np.asarray(out)
    assert out.dtype == q0.dtype
    return out


def linear5(q0, q1, q2, q3, q4):
    """the fifth-order value W5V tends to where the smoothness inputs are constant: tau = 0, so a_s = K_s * (1 + 0)"""
    T = q0.dtype.type
    K = lambda n, d: T(n) / T(d)                                   # noqa: E731
    with np.errstate(all="ignore"):
        p2 = (K(1, 3) * q0 - K(7, 6) * q1) + K(11, 6) * q2
        p1 = (K(5, 6) * q2 - K(1, 6) * q1) + K(1, 3) * q3
        p0 = (K(1, 3) * q2 + K(5, 6) * q3) - K(1, 6) * q4
        return ((K(3, 10) * p0 + K(3, 5) * p1) + K(1, 10) * p2) / ((K(3, 10) + K(3, 5)) + K(1, 10))


def ub(u, size, halo, di, dj):
    """UB at the nodes (i + di, j + dj) of the levels 1..Nz, (Nz, Ny, Nx)"""
    with np.errstate(all="ignore"):
        return u.dtype.type(0.5) * (_win(u, size, halo, di, dj - 1) + _win(u, size, halo, di, dj))


def vb(v, size, halo, di, dj):
    """VB at the nodes (i + di, j + dj) of the levels 1..Nz, (Nz, Ny, Nx)"""
    with np.errstate(all="ignore"):
        return v.dtype.type(0.5) * (_win(v, size, halo, di - 1, dj) + _win(v, size, halo, di, dj))


def upwind_vs(vel, z, a, b):
    """vel >= 0 ? W5V(z[0..4]; a[0..4]; b[0..4]) : W5V(z[5..1]; a[5..1]; b[5..1]) for the six values at -2..+3: fifteen selects, one W5V"""
    pos = vel >= 0                                                 # True for -0, False for NaN
    pick = lambda x: [np.where(pos, x[n], x[5 - n]) for n in range(5)]          # noqa: E731
    return face_value_vs(pick(z), pick(a), pick(b))


def terms(u, v, w, m, dz_c, size, halo):
    """weno_vi_ref.terms with zru, zrv, hu, hv of this rule and Gu, Gv recomposed in the rule's order; each (Nz, Ny, Nx), unmasked"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    t = dict(weno_vi_ref.terms(u, v, w, m, dz_c, size, halo))      # vu, bu, vv (vvert), bv: the one statement
    vhat, uhat = weno_momentum_ref.transverse(u, v, m, size, halo)
    Z = lambda di, dj: weno_momentum_ref.zeta_at(u, v, m, size, halo, di, dj)   # noqa: E731
    with np.errstate(all="ignore"):
        zru = upwind_vs(vhat, [Z(0, dj) for dj in range(-2, 4)], [ub(u, size, halo, 0, dj) for dj in range(-2, 4)],
                        [vb(v, size, halo, 0, dj) for dj in range(-2, 4)])
        zrv = upwind_vs(uhat, [Z(di, 0) for di in range(-2, 4)], [ub(u, size, halo, di, 0) for di in range(-2, 4)],
                        [vb(v, size, halo, di, 0) for di in range(-2, 4)])
        hu = -(vhat * zru)
        hv = uhat * zrv
        Gu = -((hu + t["vu"]) + t["bu"])
        Gv = -((hv + t["vv"]) + t["bv"])
    t.update({"vhat": vhat, "uhat": uhat, "zru": zru, "zrv": zrv, "hu": hu, "hv": hv, "Gu": Gu, "Gv": Gv})
    assert all(t[k].dtype == u.dtype and t[k].shape == (Nz, Ny, Nx) for k in ("vhat", "uhat", "zru", "zrv", "hu", "hv", "Gu", "Gv"))
    return t


def tendencies(u, v, w, Gu0, Gv0, m, dz_c, size, halo, n_fc=None, n_cf=None, mask_value=0.0):
    """the parents of (Gu, Gv) after the call: copies of `Gu0`, `Gv0` with the interior replaced, halo cells untouched"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert (n_fc is None) == (n_cf is None)
    t = terms(u, v, w, m, dz_c, size, halo)
    out = []
    for G, G0, n in zip((t["Gu"], t["Gv"]), (Gu0, Gv0), (n_fc, n_cf)):
        if n is not None:
            assert n.shape == (Ny, Nx)
            k = np.arange(1, Nz + 1)[:, None, None]
            G = np.where(k <= np.minimum(np.maximum(n.astype(np.int64), 0), Nz)[None], u.dtype.type(mask_value), G)
        assert G0.shape == u.shape
        o = G0.copy()
        o[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = G
        out.append(o)
    return tuple(out)
