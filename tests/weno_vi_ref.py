"""Host reference of the vector-invariant advection tendency of the horizontal velocities with upwinding in every term but the smoothness
stencil of the vorticity -- the WENO5 vorticity flux, the upwinded vertical (divergence and z-flux) term and the upwinded kinetic-energy
gradient -- in numpy, on padded parents: a statement of the rule of include/tripolar_hip_weno_vi.h written from the header's text.

[recalled: Oceananigans' VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(), vertical_scheme =
WENO(order = 5), kinetic_energy_gradient_scheme = WENO(order = 5), divergence_scheme = WENO(order = 5), upwinding =
OnlySelfUpwinding(cross_scheme = WENO(order = 5))); parity unpinned, like every operator here]

Taken from the existing references, the one statement of each: Z, hu and hv (weno_momentum_ref.terms), R5 (weno_ref.face_value), R3 and the
order table of the z-faces (weno_xyz_ref.face_value3, face_order).  New here, in the field type T, in exactly this order:
    C4(a, b, c, d) = (T(7)/T(12)) * (b + c) - (T(1)/T(12)) * (a + d)
    W5F(q0..q4; s0..s4) = R5 with its smoothness indicators b2, b1, b0 formed from s0..s4 and p2, p1, p0 from q0..q4
    ZF(x, M, f) = the z-face value of weno_xyz_ref at face f of the column x with M in place of Mz
    FX = Q * dz_c[k]    FY = P * dz_c[k]    DU = FX[i+1] - FX[i]    DV = FY[j+1] - FY[j]    DS = DU + DV
    HU = T(0.5) * (u*u)    HV = T(0.5) * (v*v)
    DKU = HU[i+1] - HU[i]    DKV = HV[j+1] - HV[j]    XKV = HV[i] - HV[i-1]    XKU = HU[j] - HU[j-1]
    SU = T(0.5) * (u[i] + u[i+1])    SV = T(0.5) * (v[j] + v[j+1])
 u: dvs = C4(DV[i-2..i+1, j])
    dur = uu >= 0 ? W5F(DU[i-3..i+1, j]; DS[i-3..i+1, j]) : W5F(DU[i+2..i-2, j]; DS[i+2..i-2, j])
    Wu[f] = C4(A[i-2..i+1, j, f]);   FZu[f] = Wu * ZF(u[i,j,.], Wu, f)
    vu  = (uu * (dvs + dur) + (FZu[k+1] - FZu[k])) / (az_fc[i,j] * dz_c[k])
    kus = C4(XKV[i, j-1..j+2])
    kur = uu >= 0 ? W5F(DKU[i-3..i+1, j]; SU[i-3..i+1, j]) : W5F(DKU[i+2..i-2, j]; SU[i+2..i-2, j])
    bu  = (kur + kus) / dx_fc[i,j];   Gu = -((hu + vu) + bu)
 v: the mirror image (see the header).
`>= 0` is true for -0 and false for NaN: the inputs are selected, W5F is evaluated once.  Hx, Hy >= 3, Hz >= 1.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1]; w's parent has Nz + 1 + 2 Hz planes.  numpy's elementwise arithmetic in a dtype is
one correctly rounded IEEE operation per operation: the reference is exact, comparisons are bit for bit."""
import numpy as np

import momentum_ref
import weno_momentum_ref
import weno_xyz_ref
from momentum_ref import METRICS, _win, same_bits  # noqa: F401  (same_bits re-exported: the comparison every test of this operator uses)
from weno_ref import face_value
from weno_xyz_ref import face_order  # noqa: F401  (re-exported: the order table)


def c4(a, b, c, d):
    """C4(a, b, c, d): the symmetric fourth-order value between b and c"""
    T = b.dtype.type
    with np.errstate(all="ignore"):
        out = (T(7) / T(12)) * (b + c) - (T(1) / T(12)) * (a + d)
    assert out.dtype == b.dtype
    return out


def face_value_fs(q, s):
    """W5F(q[0..4]; s[0..4]) on arrays of one floating dtype, operation for operation: weno_ref.face_value with the smoothness indicators
    formed from s"""
    q0, q1, q2, q3, q4 = q
    t0, t1, t2, t3, t4 = s
    T = q0.dtype.type
    K = lambda n, d: T(n) / T(d)                                   # noqa: E731
    eps = T(1e-8)
    S = lambda a, b, c: (a - T(2) * b) + c                         # noqa: E731
    with np.errstate(all="ignore"):
        p2 = (K(1, 3) * q0 - K(7, 6) * q1) + K(11, 6) * q2
        p1 = (K(5, 6) * q2 - K(1, 6) * q1) + K(1, 3) * q3
        p0 = (K(1, 3) * q2 + K(5, 6) * q3) - K(1, 6) * q4
        s2, d2 = S(t0, t1, t2), (t0 - T(4) * t1) + T(3) * t2
        s1, d1 = S(t1, t2, t3), t1 - t3
        s0, d0 = S(t2, t3, t4), (T(3) * t2 - T(4) * t3) + t4
        b2 = K(13, 12) * (s2 * s2) + T(0.25) * (d2 * d2)
        b1 = K(13, 12) * (s1 * s1) + T(0.25) * (d1 * d1)
        b0 = K(13, 12) * (s0 * s0) + T(0.25) * (d0 * d0)
        tau = np.abs(b0 - b2)
        r0, r1, r2 = tau / (b0 + eps), tau / (b1 + eps), tau / (b2 + eps)
        a0, a1, a2 = K(3, 10) * (T(1) + r0 * r0), K(3, 5) * (T(1) + r1 * r1), K(1, 10) * (T(1) + r2 * r2)
        out = ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2)
    assert out.dtype == q0.dtype
    return out


def upwind_fs(vel, q, s):
    """vel >= 0 ? W5F(q[0..4]; s[0..4]) : W5F(q[5..1]; s[5..1]) for the six values q[0..5], s[0..5] at -3..+2 of the face: ten selects, one
    W5F"""
    pos = vel >= 0                                                 # True for -0, False for NaN
    return face_value_fs([np.where(pos, q[n], q[5 - n]) for n in range(5)], [np.where(pos, s[n], s[5 - n]) for n in range(5)])


def z_face_values(x, M, size, halo):
    """ZF(x[i,j,.], M[i,j,f], f) at the Nz + 1 faces of the interior columns, (Nz + 1, Ny, Nx): weno_xyz_ref's, the one statement"""
    return weno_xyz_ref.z_face_values(x, M, size, halo)


# ---- the stencil, derived from the rule: (array, di, dj, dk) of every cell a node (i, j, k) reads ------------------------------------------
_Q = lambda di, dj: (("dy_fc", di, dj, 0), ("u", di, dj, 0))                                                                  # noqa: E731
_P = lambda di, dj: (("dx_cf", di, dj, 0), ("v", di, dj, 0))                                                                  # noqa: E731
_DU = lambda di, dj: (*_Q(di + 1, dj), *_Q(di, dj))                                                                           # noqa: E731
_DV = lambda di, dj: (*_P(di, dj + 1), *_P(di, dj))                                                                           # noqa: E731
_A = lambda di, dj: tuple(x for dk in (0, 1) for x in (("az_cc", di, dj, 0), ("w", di, dj, dk)))                              # noqa: E731
# the z-arm of the advected velocity itself is written from the order table (cells_read, dependence), not listed per node
_NEW_U = (*(c for di in range(-2, 2) for c in _DV(di, 0)), *(c for di in range(-3, 3) for c in (*_DU(di, 0), *_DV(di, 0))),
          *(c for di in range(-2, 2) for c in _A(di, 0)), ("az_fc", 0, 0, 0), ("dx_fc", 0, 0, 0),
          *(("v", di, dj, 0) for di in (-1, 0) for dj in range(-1, 3)), *(("u", di, 0, 0) for di in range(-3, 4)))
_NEW_V = (*(c for dj in range(-2, 2) for c in _DU(0, dj)), *(c for dj in range(-3, 3) for c in (*_DU(0, dj), *_DV(0, dj))),
          *(c for dj in range(-2, 2) for c in _A(0, dj)), ("az_cf", 0, 0, 0), ("dy_cf", 0, 0, 0),
          *(("u", di, dj, 0) for dj in (-1, 0) for di in range(-1, 3)), *(("v", 0, dj, 0) for dj in range(-3, 4)))
# of the built vorticity rule only hu, hv stay: Z's windows, vh, uh and their divisors (K, S, R and their cells go)
_HU = tuple(sorted({c for dj in range(-2, 4) for c in momentum_ref._Z(0, dj)} | {c for di in (-1, 0) for dj in (0, 1) for c in _P(di, dj)}
                   | {("dx_fc", 0, 0, 0)}))
_HV = tuple(sorted({c for di in range(-2, 4) for c in momentum_ref._Z(di, 0)} | {c for di in (0, 1) for dj in (-1, 0) for c in _Q(di, dj)}
                   | {("dy_cf", 0, 0, 0)}))
STENCIL_U = tuple(sorted(set(_HU) | set(_NEW_U)))
STENCIL_V = tuple(sorted(set(_HV) | set(_NEW_V)))
STENCIL = tuple(sorted(set(STENCIL_U) | set(STENCIL_V)))


def _levels(a, size, halo, nz=None):
    """the planes of the levels 1..nz (default Nz) of a parent, whole planes: (nz, sy, sx)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return a[Hz:Hz + (Nz if nz is None else nz)]


def _sh(a, di=0, dj=0):
    """the array whose cell (i, j) is a's (i + di, j + dj), whole planes.  The roll wraps at the parent's edge: every quantity below is
    used at most three cells beyond the interior, where nothing wrapped arrives (Hx, Hy >= 3; test_weno_vi_ref.py finds the cells read by
    perturbing every cell)"""
    return np.roll(a, (-dj, -di), axis=(-2, -1))


def terms(u, v, w, m, dz_c, size, halo):
    """every named quantity of the rule on the interior, each (Nz, Ny, Nx) (FZu, FZv, Wu, Wv: (Nz + 1, Ny, Nx)), unmasked"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    T = u.dtype
    assert Hx >= 3 and Hy >= 3 and Hz >= 1 and dz_c.shape == (Nz,) and dz_c.dtype == T
    half = T.type(0.5)
    old = weno_momentum_ref.terms(u, v, w, m, np.ones(Nz + 1, T), size, halo)    # hu, hv: the built vorticity term (dz_f does not enter them)
    I = lambda a: a[..., Hy:Hy + Ny, Hx:Hx + Nx]                                   # noqa: E731,E741
    with np.errstate(all="ignore"):
        d = dz_c[:, None, None]
        ul, vl = _levels(u, size, halo), _levels(v, size, halo)
        FX = (m["dy_fc"][None] * ul) * d
        FY = (m["dx_cf"][None] * vl) * d
        DU = _sh(FX, 1, 0) - FX
        DV = _sh(FY, 0, 1) - FY
        DS = DU + DV
        HU = half * (ul * ul)
        HV = half * (vl * vl)
        DKU = _sh(HU, 1, 0) - HU
        DKV = _sh(HV, 0, 1) - HV
        XKV = HV - _sh(HV, -1, 0)
        XKU = HU - _sh(HU, 0, -1)
        SU = half * (ul + _sh(ul, 1, 0))
        SV = half * (vl + _sh(vl, 0, 1))
        A = m["az_cc"][None] * _levels(w, size, halo, Nz + 1)      # faces 1..Nz+1
        uu, vv = I(ul), I(vl)
        # u
        dvs = c4(*(I(_sh(DV, di, 0)) for di in range(-2, 2)))
        dur = upwind_fs(uu, [I(_sh(DU, di, 0)) for di in range(-3, 3)], [I(_sh(DS, di, 0)) for di in range(-3, 3)])
        Wu = c4(*(I(_sh(A, di, 0)) for di in range(-2, 2)))
        FZu = Wu * z_face_values(u, Wu, size, halo)
        vu = (uu * (dvs + dur) + (FZu[1:] - FZu[:-1])) / (I(m["az_fc"])[None] * d)
        kus = c4(*(I(_sh(XKV, 0, dj)) for dj in range(-1, 3)))
        kur = upwind_fs(uu, [I(_sh(DKU, di, 0)) for di in range(-3, 3)], [I(_sh(SU, di, 0)) for di in range(-3, 3)])
        bu = (kur + kus) / I(m["dx_fc"])[None]
        Gu = -((old["hu"] + vu) + bu)
        # v
        dus = c4(*(I(_sh(DU, 0, dj)) for dj in range(-2, 2)))
        dvr = upwind_fs(vv, [I(_sh(DV, 0, dj)) for dj in range(-3, 3)], [I(_sh(DS, 0, dj)) for dj in range(-3, 3)])
        Wv = c4(*(I(_sh(A, 0, dj)) for dj in range(-2, 2)))
        FZv = Wv * z_face_values(v, Wv, size, halo)
        vvert = (vv * (dus + dvr) + (FZv[1:] - FZv[:-1])) / (I(m["az_cf"])[None] * d)
        kvs = c4(*(I(_sh(XKU, di, 0)) for di in range(-1, 3)))
        kvr = upwind_fs(vv, [I(_sh(DKV, 0, dj)) for dj in range(-3, 3)], [I(_sh(SV, 0, dj)) for dj in range(-3, 3)])
        bv = (kvr + kvs) / I(m["dy_cf"])[None]
        Gv = -((old["hv"] + vvert) + bv)
    out = {"hu": old["hu"], "hv": old["hv"], "dvs": dvs, "dur": dur, "vu": vu, "kus": kus, "kur": kur, "bu": bu, "Gu": Gu,
           "dus": dus, "dvr": dvr, "vv": vvert, "kvs": kvs, "kvr": kvr, "bv": bv, "Gv": Gv}
    assert all(a.dtype == T and a.shape == (Nz, Ny, Nx) for a in out.values())
    out.update({"Wu": Wu, "Wv": Wv, "FZu": FZu, "FZv": FZv})
    assert all(out[k].dtype == T and out[k].shape == (Nz + 1, Ny, Nx) for k in ("Wu", "Wv", "FZu", "FZv"))
    return out


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


def z_planes_read(size, halo):
    """the planes of a parent of u or v that some z-face of an interior column reads, boolean (Nz + 2 Hz,): 0 .. Nz + 1, from the order table"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    planes = np.zeros(Nz + 2 * Hz, bool)
    for f in range(1, Nz + 2):
        order = face_order(f, Nz)
        lo, hi = {weno_xyz_ref.CENTRED: (f - 1, f), 1: (f - 1, f), 3: (f - 2, f + 1), 5: (f - 3, f + 2)}[order]
        assert order == weno_xyz_ref.CENTRED or (lo >= 1 and hi <= Nz)
        planes[Hz + lo - 1:Hz + hi] = True
    return planes


def cells_read(size, halo):
    """boolean masks of the cells the rule reads, whichever way the flow goes: STENCIL at the levels 1..Nz, and the interior columns of u
    and v at the planes 0 .. Nz + 1 (the z-arm).  {"u", "v": parent-shaped; "w": its own longer parent; the eight metric names:
    plane-shaped}"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    read = momentum_ref.cells_read(size, halo, STENCIL)
    planes = z_planes_read(size, halo)
    for name in ("u", "v"):
        read[name][:, Hy:Hy + Ny, Hx:Hx + Nx] |= planes[:, None, None]
    return read


# ---- the domain of dependence, by the signs of the flow ---------------------------------------------------------------------------------------
_LEFT = {True: range(-3, 2), False: range(-2, 3)}                  # the cells of a W5F window around a face, by the sign of the advected velocity
_ZWIN = {True: range(-2, 3), False: range(-1, 4)}                  # the Z of a vorticity window, by the sign of the transverse velocity


def stencil_u(u_positive, v_positive):
    """(array, di, dj, 0) of every cell of the node's level that Gu reads when uu has one sign and vhat has one"""
    cells = {c for dj in _ZWIN[v_positive] for c in momentum_ref._Z(0, dj)} | {c for di in (-1, 0) for dj in (0, 1) for c in _P(di, dj)}
    cells |= {c for di in range(-2, 2) for c in _DV(di, 0)} | {c for di in _LEFT[u_positive] for c in (*_DU(di, 0), *_DV(di, 0))}
    cells |= {("v", di, dj, 0) for di in (-1, 0) for dj in range(-1, 3)} | {("u", di + o, 0, 0) for di in _LEFT[u_positive] for o in (0, 1)}
    return tuple(sorted(cells | {("u", 0, 0, 0)}))


def stencil_v(u_positive, v_positive):
    cells = {c for di in _ZWIN[u_positive] for c in momentum_ref._Z(di, 0)} | {c for di in (0, 1) for dj in (-1, 0) for c in _Q(di, dj)}
    cells |= {c for dj in range(-2, 2) for c in _DU(0, dj)} | {c for dj in _LEFT[v_positive] for c in (*_DU(0, dj), *_DV(0, dj))}
    cells |= {("u", di, dj, 0) for dj in (-1, 0) for di in range(-1, 3)} | {("v", 0, dj + o, 0) for dj in _LEFT[v_positive] for o in (0, 1)}
    return tuple(sorted(cells | {("v", 0, 0, 0)}))


def z_levels_read(k, Nz, w_positive):
    """the levels (0 .. Nz + 1) of its own column that node k = 1..Nz reads through its faces k and k + 1 when Wu (Wv) has one sign"""
    out = set()
    for f in (k, k + 1):
        order = face_order(f, Nz)
        if order == weno_xyz_ref.CENTRED:
            out |= {f - 1, f}
        elif order == 1:
            out |= {f - 1} if w_positive else {f}
        elif order == 3:
            out |= {f - 2, f - 1, f} if w_positive else {f + 1, f, f - 1}
        else:
            out |= set(range(f - 3, f + 2)) if w_positive else set(range(f - 2, f + 3))
    return out


def dependence_window(name, changed, size, halo, u_positive, v_positive, w_positive):
    """The interior nodes of (Gu, Gv) that may change when the cells `changed` (a boolean parent of `name`, "u" or "v", halos included)
    change while u, v and w have one sign each everywhere (so uu and uhat have u's, vv and vhat v's, Wu and Wv w's): a node reads the cell
    (i + di, j + dj, k) for every entry of its stencil and the levels z_levels_read of its own column.  Returns two boolean (Nz, Ny, Nx)."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    out = []
    for own, stencil in (("u", stencil_u(u_positive, v_positive)), ("v", stencil_v(u_positive, v_positive))):
        reach = np.zeros((Nz, Ny, Nx), bool)
        for arr, di, dj, dk in stencil:
            if arr == name:
                reach |= _win(changed, size, halo, di, dj, dk)
        if own == name:
            for k in range(1, Nz + 1):
                for level in z_levels_read(k, Nz, w_positive):
                    reach[k - 1] |= changed[Hz + level - 1, Hy:Hy + Ny, Hx:Hx + Nx]
        out.append(reach)
    return tuple(out)
