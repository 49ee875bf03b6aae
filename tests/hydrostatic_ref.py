"""Host reference of the Coriolis and hydrostatic pressure-gradient tendencies of the horizontal velocities (and of the hydrostatic pressure
anomaly) in numpy, on padded parents: the rule of include/tripolar_hip_hydrostatic.h [recalled: Oceananigans' update_hydrostatic_pressure!,
d/dx of pHY' and x_f_cross_U / y_f_cross_U of HydrostaticSphericalCoriolis; parity unpinned, like every operator here].

    PH[i,j,Nz] = -((T(0.5) * (b[i,j,Nz] + b[i,j,Nz+1])) * dz_f[Nz+1])
    PH[i,j,k]  = PH[i,j,k+1] - ((T(0.5) * (b[i,j,k] + b[i,j,k+1])) * dz_f[k+1])        k = Nz-1 .. 1, in this order
    px = (PH[i,j,k] - PH[i-1,j,k]) / dx_fc[i,j]          py = (PH[i,j,k] - PH[i,j-1,k]) / dy_cf[i,j]
    P[i,j,k] = dx_cf[i,j] * v[i,j,k]     Q[i,j,k] = dy_fc[i,j] * u[i,j,k]      (momentum_ref's P, Q: its windows, its stencils)
  ENSTROPHY (0):
    fb = T(0.5) * (f_ff[i,j] + f_ff[i,j+1]);  vh = T(0.5) * (T(0.5) * (P[i-1,j,k] + P[i-1,j+1,k]) + T(0.5) * (P[i,j,k] + P[i,j+1,k]))
    cu = (fb * vh) / dx_fc[i,j]
    fb = T(0.5) * (f_ff[i,j] + f_ff[i+1,j]);  uh = T(0.5) * (T(0.5) * (Q[i,j-1,k] + Q[i+1,j-1,k]) + T(0.5) * (Q[i,j,k] + Q[i+1,j,k]))
    cv = (fb * uh) / dy_cf[i,j]
  ENERGY (1):
    VX[i,j,k] = T(0.5) * (P[i-1,j,k] + P[i,j,k]);   cu = (T(0.5) * (f_ff[i,j] * VX[i,j,k] + f_ff[i,j+1] * VX[i,j+1,k])) / dx_fc[i,j]
    UY[i,j,k] = T(0.5) * (Q[i,j-1,k] + Q[i,j,k]);   cv = (T(0.5) * (f_ff[i,j] * UY[i,j,k] + f_ff[i+1,j] * UY[i+1,j,k])) / dy_cf[i,j]
  ADD (0):    Gu = (Gu + cu) - px      Gv = (Gv - cv) - py          WRITE (1):  Gu = cu - px      Gv = (-cv) - py
  a dropped term (f None, or b None) is omitted: Gu + cu, Gv - cv, cu, -cv; or Gu - px, Gv - py, -px, -py.
Mask: with n_fc, n_cf the nodes k <= min(max(n, 0), Nz) of Gu, Gv hold T(mask_value) in both modes; p is never masked.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1], planes [j + Hy - 1, i + Hx - 1].  Every operation is one correctly rounded IEEE
operation of the element type, which numpy's elementwise arithmetic in that dtype is too: comparisons are bit for bit."""
import numpy as np

from momentum_ref import _P, _Q, _win
from vorticity_ref import same_bits  # noqa: F401  (re-exported)

ENSTROPHY, ENERGY = 0, 1
ADD, WRITE = 0, 1
METRICS = ("dx_fc", "dy_fc", "dx_cf", "dy_cf")

# the stencil in the plane, (array, di, dj, 0) as momentum_ref writes them: what a node (i, j) reads for Gu and for Gv.  b apart: b_columns
CORIOLIS_U = (*_P(-1, 0), *_P(-1, 1), *_P(0, 0), *_P(0, 1), ("f_ff", 0, 0, 0), ("f_ff", 0, 1, 0), ("dx_fc", 0, 0, 0))
CORIOLIS_V = (*_Q(0, -1), *_Q(1, -1), *_Q(0, 0), *_Q(1, 0), ("f_ff", 0, 0, 0), ("f_ff", 1, 0, 0), ("dy_cf", 0, 0, 0))
PRESSURE_U = (("b", 0, 0), ("b", -1, 0), ("dx_fc", 0, 0, 0))
PRESSURE_V = (("b", 0, 0), ("b", 0, -1), ("dy_cf", 0, 0, 0))


def pressure_columns(b, dz_f, size, halo):
    """PH at the levels k = 1..Nz of EVERY column of the parent, halo columns included: (Nz, Ny + 2 Hy, Nx + 2 Hx), in the dtype of b"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    T = b.dtype.type
    assert dz_f.shape == (Nz + 1,) and dz_f.dtype == b.dtype and Hz >= 1 and b.shape == (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    half = T(0.5)
    PH = np.empty((Nz,) + b.shape[1:], b.dtype)
    with np.errstate(all="ignore"):
        for k in range(Nz, 0, -1):                                 # 1-based level k is parent plane k + Hz - 1
            x = (half * (b[k + Hz - 1] + b[k + Hz])) * dz_f[k]     # dz_f[k + 1], 1-based, is element k
            PH[k - 1] = -x if k == Nz else PH[k] - x
    return PH


def pressure_gradient(b, m, dz_f, size, halo):
    """(px, py, PH) on the interior, each (Nz, Ny, Nx)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    PH = pressure_columns(b, dz_f, size, halo)
    W = lambda di, dj: PH[:, Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx]                                                       # noqa: E731
    with np.errstate(all="ignore"):
        px = (W(0, 0) - W(-1, 0)) / _win(m["dx_fc"], size, halo)
        py = (W(0, 0) - W(0, -1)) / _win(m["dy_cf"], size, halo)
    return px, py, W(0, 0)


def coriolis(u, v, f, m, size, halo, scheme=ENSTROPHY):
    """(cu, cv) on the interior, each (Nz, Ny, Nx), in the dtype of u"""
    T = u.dtype.type
    assert v.dtype == u.dtype == f.dtype and all(m[k].dtype == u.dtype for k in METRICS) and scheme in (ENSTROPHY, ENERGY)
    half = T(0.5)
    W = lambda p, di=0, dj=0: _win(p, size, halo, di, dj)                                                                      # noqa: E731
    with np.errstate(all="ignore"):
        P = lambda di, dj: W(m["dx_cf"], di, dj) * W(v, di, dj)                                                                # noqa: E731
        Q = lambda di, dj: W(m["dy_fc"], di, dj) * W(u, di, dj)                                                                # noqa: E731
        if scheme == ENSTROPHY:
            fb = half * (W(f) + W(f, 0, 1))
            vh = half * (half * (P(-1, 0) + P(-1, 1)) + half * (P(0, 0) + P(0, 1)))
            cu = (fb * vh) / W(m["dx_fc"])
            fb = half * (W(f) + W(f, 1, 0))
            uh = half * (half * (Q(0, -1) + Q(1, -1)) + half * (Q(0, 0) + Q(1, 0)))
            cv = (fb * uh) / W(m["dy_cf"])
        else:
            VX = lambda dj: half * (P(-1, dj) + P(0, dj))                                                                      # noqa: E731
            cu = (half * (W(f) * VX(0) + W(f, 0, 1) * VX(1))) / W(m["dx_fc"])
            UY = lambda di: half * (Q(di, -1) + Q(di, 0))                                                                      # noqa: E731
            cv = (half * (W(f) * UY(0) + W(f, 1, 0) * UY(1))) / W(m["dy_cf"])
    assert cu.dtype == cv.dtype == u.dtype
    return cu, cv


def interior_tendencies(u, v, b, Gu0, Gv0, f, m, dz_f, size, halo, scheme=ENSTROPHY, mode=ADD):
    """(Gu, Gv, PH or None) on the interior, unmasked; f None drops the Coriolis term, b None the pressure term"""
    assert f is not None or b is not None
    assert mode in (ADD, WRITE)
    with np.errstate(all="ignore"):
        cu = cv = px = py = PH = None
        if f is not None:
            cu, cv = coriolis(u, v, f, m, size, halo, scheme)
        if b is not None:
            px, py, PH = pressure_gradient(b, m, dz_f, size, halo)
        if mode == ADD:
            gu, gv = _win(Gu0, size, halo), _win(Gv0, size, halo)
            if f is not None and b is not None:
                return (gu + cu) - px, (gv - cv) - py, PH
            return (gu + cu, gv - cv, PH) if b is None else (gu - px, gv - py, PH)
        if f is not None and b is not None:
            return cu - px, (-cv) - py, PH
        return (cu.copy(), -cv, PH) if b is None else (-px, -py, PH)


def tendencies(u, v, b, Gu0, Gv0, p0, f, m, dz_f, size, halo, scheme=ENSTROPHY, mode=ADD, n_fc=None, n_cf=None, mask_value=0.0):
    """the parents of (Gu, Gv, p) after the call: copies of Gu0, Gv0, p0 with the interior replaced, halo cells untouched.  p0 None: no
    p_out, None comes back.  Gu0 and Gv0 None: the pressure alone"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert (n_fc is None) == (n_cf is None) and min(halo) >= 1
    inner = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    if Gu0 is None:
        assert Gv0 is None and b is not None and p0 is not None
        p = p0.copy()
        p[inner] = pressure_columns(b, dz_f, size, halo)[:, Hy:Hy + Ny, Hx:Hx + Nx]
        return None, None, p
    Gu, Gv, PH = interior_tendencies(u, v, b, Gu0, Gv0, f, m, dz_f, size, halo, scheme, mode)
    out = []
    for G, G0, n in ((Gu, Gu0, n_fc), (Gv, Gv0, n_cf)):
        if n is not None:
            assert n.shape == (Ny, Nx)
            k = np.arange(1, Nz + 1)[:, None, None]
            G = np.where(k <= np.minimum(np.maximum(n.astype(np.int64), 0), Nz)[None], G0.dtype.type(mask_value), G)
        o = G0.copy()
        o[inner] = G
        out.append(o)
    p = None
    if p0 is not None:
        assert PH is not None
        p = p0.copy()
        p[inner] = PH
    return out[0], out[1], p


def cells_read(size, halo, coriolis=True, pressure=True, which="both"):
    """boolean masks of the cells the rule reads for `which` ("Gu", "Gv", "both", or "p": p_out alone), derived from the stencils above:
    {"u", "v", "b": parent-shaped; "f_ff" and the four metric names: plane-shaped}.  b is read at (di, dj) on every level 1 .. Nz + 1"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    plane, parent = (Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    read = {k: np.zeros(parent, bool) for k in ("u", "v", "b")}
    read.update({k: np.zeros(plane, bool) for k in ("f_ff", *METRICS)})
    stencil = []
    if which == "p":
        stencil = [("b", 0, 0)]
    else:
        for name, cor, pres in (("Gu", CORIOLIS_U, PRESSURE_U), ("Gv", CORIOLIS_V, PRESSURE_V)):
            if which in (name, "both"):
                stencil += (list(cor) if coriolis else []) + (list(pres) if pressure else [])
    for name, di, dj, *_ in stencil:
        if name == "b":
            read["b"][Hz:Hz + Nz + 1, Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx] = True
        else:
            _win(read[name], size, halo, di, dj)[...] = True
    return read
