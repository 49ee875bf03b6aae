"""Host reference of the vector-invariant advection tendency of the horizontal velocities with the WENO5-upwinded vorticity term in numpy,
on padded parents: a statement of the rule of include/tripolar_hip_weno_momentum.h written from the header's text.

[recalled: Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(), vertical_scheme =
EnergyConserving()); parity unpinned, like every operator here]

Everything not named here is momentum_ref's, with the same bits: Z (momentum_ref.zeta, the one statement), vu, bu, vv, bv
(momentum_ref.terms, the one statement), the mask.  W5 is weno_ref.face_value, the one statement.  Only hu and hv are replaced:
    u: vhat = vh / dx_fc[i,j]
       zr   = vhat >= 0 ? W5(Z[i,j-2], Z[i,j-1], Z[i,j],   Z[i,j+1], Z[i,j+2]) : W5(Z[i,j+3], Z[i,j+2], Z[i,j+1], Z[i,j],   Z[i,j-1])
       hu   = -(vhat * zr);   Gu = -((hu + vu) + bu)
    v: uhat = uh / dy_cf[i,j]
       zr   = uhat >= 0 ? W5(Z[i-2,j], Z[i-1,j], Z[i,j],   Z[i+1,j], Z[i+2,j]) : W5(Z[i+3,j], Z[i+2,j], Z[i+1,j], Z[i,j],   Z[i-1,j])
       hv   = uhat * zr;      Gv = -((hv + vv) + bv)
with vh = T(0.5) * (T(0.5) * (P[i-1,j] + P[i-1,j+1]) + T(0.5) * (P[i,j] + P[i,j+1])), P = dx_cf * v, and
uh = T(0.5) * (T(0.5) * (Q[i,j-1] + Q[i+1,j-1]) + T(0.5) * (Q[i,j] + Q[i+1,j])), Q = dy_fc * u, as in momentum_ref's rule (terms() does not
give them out, so they are written again here, operation for operation).  `>= 0` is true for -0 and false for NaN: five inputs are
selected, W5 is evaluated once.  Hx, Hy >= 3, Hz >= 1.  Only interior cells of Gu, Gv are written.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1].  numpy's elementwise arithmetic in a dtype is one correctly rounded IEEE operation
per operation: the reference is exact, comparisons are bit for bit."""
import numpy as np

import momentum_ref
from momentum_ref import METRICS, _win, same_bits  # noqa: F401  (same_bits re-exported: the comparison every test of this operator uses)
from weno_ref import face_value

_Z = momentum_ref._Z
_UP = {True: range(-2, 3), False: range(-1, 4)}                    # the Z a window holds, by the sign of the transverse velocity (>= 0: True)


def stencil_u(positive=None):
    """(array, di, dj, dk) of every cell a node reads for Gu: momentum_ref's, and Z[i, j-2..j+3] (positive None: both windows)"""
    rows = range(-2, 4) if positive is None else _UP[positive]
    return tuple(sorted(set(momentum_ref.STENCIL_U) | {c for dj in rows for c in _Z(0, dj)}))


def stencil_v(positive=None):
    rows = range(-2, 4) if positive is None else _UP[positive]
    return tuple(sorted(set(momentum_ref.STENCIL_V) | {c for di in rows for c in _Z(di, 0)}))


STENCIL = tuple(sorted(set(stencil_u()) | set(stencil_v())))


def _shifted(a, di, dj):
    """the array whose cell (i, j) is a's (i + di, j + dj): only cells well inside the parent are used by the callers (asserted there)"""
    return np.roll(a, (-dj, -di), axis=(-2, -1))


def zeta_at(u, v, m, size, halo, di, dj):
    """momentum_ref.zeta -- the one statement of Z -- at the nodes (i + di, j + dj), (Nz, Ny, Nx)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert 1 - Hx <= di <= Hx and 1 - Hy <= dj <= Hy               # Z reads one cell further west and south: the roll wraps nothing in
    ms = {k: _shifted(m[k], di, dj) for k in ("dy_cf", "dx_fc", "az_ff")}
    return momentum_ref.zeta(_shifted(u, di, dj), _shifted(v, di, dj), ms, size, halo)


def upwind(vel, z):
    """vel >= 0 ? W5(z[0..4]) : W5(z[5], z[4], z[3], z[2], z[1]) for the six values z[0..5] = Z[-2..+3]: five selects, one W5"""
    pos = vel >= 0                                                 # True for -0, False for NaN
    return face_value(*(np.where(pos, z[n], z[5 - n]) for n in range(5)))


def transverse(u, v, m, size, halo):
    """(vhat, uhat) on the interior, each (Nz, Ny, Nx)"""
    T = u.dtype
    half = T.type(0.5)
    W = lambda p, di=0, dj=0: _win(p, size, halo, di, dj)                                                                      # noqa: E731
    with np.errstate(all="ignore"):
        P = lambda di, dj: W(m["dx_cf"], di, dj) * W(v, di, dj)                                                                # noqa: E731
        Q = lambda di, dj: W(m["dy_fc"], di, dj) * W(u, di, dj)                                                                # noqa: E731
        vh = half * (half * (P(-1, 0) + P(-1, 1)) + half * (P(0, 0) + P(0, 1)))
        uh = half * (half * (Q(0, -1) + Q(1, -1)) + half * (Q(0, 0) + Q(1, 0)))
        return vh / W(m["dx_fc"]), uh / W(m["dy_cf"])


def terms(u, v, w, m, dz_f, size, halo):
    """{"vhat", "uhat", "zru", "zrv", "hu", "vu", "bu", "hv", "vv", "bv", "Gu", "Gv"} on the interior, each (Nz, Ny, Nx), unmasked"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert Hx >= 3 and Hy >= 3 and Hz >= 1
    t = momentum_ref.terms(u, v, w, m, dz_f, size, halo)           # vu, bu, vv, bv: the one statement
    vhat, uhat = transverse(u, v, m, size, halo)
    with np.errstate(all="ignore"):
        zru = upwind(vhat, [zeta_at(u, v, m, size, halo, 0, dj) for dj in range(-2, 4)])
        zrv = upwind(uhat, [zeta_at(u, v, m, size, halo, di, 0) for di in range(-2, 4)])
        hu = -(vhat * zru)
        hv = uhat * zrv
        Gu = -((hu + t["vu"]) + t["bu"])
        Gv = -((hv + t["vv"]) + t["bv"])
    out = {"vhat": vhat, "uhat": uhat, "zru": zru, "zrv": zrv, "hu": hu, "vu": t["vu"], "bu": t["bu"], "hv": hv, "vv": t["vv"], "bv": t["bv"],
           "Gu": Gu, "Gv": Gv}
    assert all(a.dtype == u.dtype and a.shape == (Nz, Ny, Nx) for a in out.values())
    return out


def tendencies(u, v, w, Gu0, Gv0, m, dz_f, size, halo, n_fc=None, n_cf=None, mask_value=0.0):
    """the parents of (Gu, Gv) after the call: copies of `Gu0`, `Gv0` with the interior replaced, halo cells untouched"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert (n_fc is None) == (n_cf is None)
    t = terms(u, v, w, m, dz_f, size, halo)
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


def cells_read(size, halo):
    """boolean masks of the cells the rule reads, whichever way the flow goes, derived from STENCIL: {"u", "v": parent-shaped; "w": its own
    longer parent; the eight metric names: plane-shaped}"""
    return momentum_ref.cells_read(size, halo, STENCIL)


def dependence_window(name, changed, size, halo, v_positive, u_positive):
    """The interior nodes of (Gu, Gv) that may change when the cells `changed` (a boolean parent of `name`, "u" or "v", halos included)
    change while vhat has one sign everywhere (v_positive) and uhat has one (u_positive): a node (i, j, k) reads the cell
    (i + di, j + dj, k + dk) for every entry of its stencil, so a changed cell reaches the nodes cell - (di, dj, dk), no others.  Returns two
    boolean (Nz, Ny, Nx)."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    out = []
    for stencil in (stencil_u(v_positive), stencil_v(u_positive)):
        reach = np.zeros((Nz, Ny, Nx), bool)
        for arr, di, dj, dk in stencil:
            if arr == name:
                reach |= _win(changed, size, halo, di, dj, dk)
        out.append(reach)
    return tuple(out)
