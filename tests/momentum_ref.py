"""Host reference of the vector-invariant advection tendency of the horizontal velocities in numpy, on padded parents.

The rule [recalled: Oceananigans' U_dot_∇u / U_dot_∇v for VectorInvariant() with EnstrophyConserving vorticity, the ζ₂wᶠᶜᶠ / ζ₁wᶜᶠᶠ vertical
terms and ∂x Khᶜᶜᶜ; parity unpinned, like every operator here]

The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with no
contraction.  Every operation is one correctly rounded IEEE operation.  kf is a face index; w has Nz + 1 levels.
    Z[i,j,k]  = ((dy_cf[i,j] v[i,j,k] - dy_cf[i-1,j] v[i-1,j,k]) - (dx_fc[i,j] u[i,j,k] - dx_fc[i,j-1] u[i,j-1,k])) / az_ff[i,j]
    P[i,j,k]  = dx_cf[i,j] * v[i,j,k]      Q[i,j,k] = dy_fc[i,j] * u[i,j,k]      A[i,j,kf] = az_cc[i,j] * w[i,j,kf]
    K[i,j,k]  = T(0.5) * (T(0.5) * (u[i,j,k]*u[i,j,k] + u[i+1,j,k]*u[i+1,j,k]) + T(0.5) * (v[i,j,k]*v[i,j,k] + v[i,j+1,k]*v[i,j+1,k]))
 u: zb = T(0.5) * (Z[i,j,k] + Z[i,j+1,k])
    vh = T(0.5) * (T(0.5) * (P[i-1,j,k] + P[i-1,j+1,k]) + T(0.5) * (P[i,j,k] + P[i,j+1,k]))
    hu = -((zb * vh) / dx_fc[i,j])
    bu = (K[i,j,k] - K[i-1,j,k]) / dx_fc[i,j]
    S[i,j,kf] = (T(0.5) * (A[i-1,j,kf] + A[i,j,kf])) * ((u[i,j,kf] - u[i,j,kf-1]) / dz_f[kf])        kf = 1..Nz+1
    vu = (T(0.5) * (S[i,j,k] + S[i,j,k+1])) / az_fc[i,j]
    Gu[i,j,k] = -((hu + vu) + bu)
 v: zb = T(0.5) * (Z[i,j,k] + Z[i+1,j,k])
    uh = T(0.5) * (T(0.5) * (Q[i,j-1,k] + Q[i+1,j-1,k]) + T(0.5) * (Q[i,j,k] + Q[i+1,j,k]))
    hv = (zb * uh) / dy_cf[i,j]
    bv = (K[i,j,k] - K[i,j-1,k]) / dy_cf[i,j]
    R[i,j,kf] = (T(0.5) * (A[i,j-1,kf] + A[i,j,kf])) * ((v[i,j,kf] - v[i,j,kf-1]) / dz_f[kf])
    vv = (T(0.5) * (R[i,j,k] + R[i,j,k+1])) / az_cf[i,j]
    Gv[i,j,k] = -((hv + vv) + bv)
- Each of Z, P, Q, K, A, S, R has one definition.  Leading minus signs are sign flips.  A zero divisor divides, as the rule says.
- dz_f holds Nz + 1 values: the centre-to-centre spacing at faces 1..Nz+1.
- Only interior cells of Gu, Gv are written.
- Mask: with the count planes n_fc, n_cf (Ny, Nx), the nodes k <= min(max(n, 0), Nz) of Gu (by n_fc) and Gv (by n_cf) hold T(mask_value)
  instead; everything is computed unmasked (what tpg_mask_immersed_fields leaves).

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1], planes [j + Hy - 1, i + Hx - 1]; w's parent has Nz + 1 + 2 Hz planes.  Every
operation is one correctly rounded IEEE operation of the element type, which numpy's elementwise arithmetic in that dtype is too: the
reference is exact, comparisons are bit for bit."""
import numpy as np

from vorticity_ref import same_bits  # noqa: F401  (re-exported: the comparison every test of this operator uses)

METRICS = ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff")

# the stencil, derived from the rule above: (array, di, dj, dk) of every cell a node (i, j, k) reads for Gu or Gv
_Z = lambda di, dj: (("v", di, dj, 0), ("dy_cf", di, dj, 0), ("v", di - 1, dj, 0), ("dy_cf", di - 1, dj, 0),                 # noqa: E731
                     ("u", di, dj, 0), ("dx_fc", di, dj, 0), ("u", di, dj - 1, 0), ("dx_fc", di, dj - 1, 0), ("az_ff", di, dj, 0))
_K = lambda di, dj: (("u", di, dj, 0), ("u", di + 1, dj, 0), ("v", di, dj, 0), ("v", di, dj + 1, 0))                          # noqa: E731
_P = lambda di, dj: (("dx_cf", di, dj, 0), ("v", di, dj, 0))                                                                  # noqa: E731
_Q = lambda di, dj: (("dy_fc", di, dj, 0), ("u", di, dj, 0))                                                                  # noqa: E731
_A = lambda di, dj, dk: (("az_cc", di, dj, 0), ("w", di, dj, dk))                                                             # noqa: E731
STENCIL_U = (*_Z(0, 0), *_Z(0, 1), *_P(-1, 0), *_P(-1, 1), *_P(0, 0), *_P(0, 1), ("dx_fc", 0, 0, 0), *_K(0, 0), *_K(-1, 0),
             *_A(-1, 0, 0), *_A(0, 0, 0), *_A(-1, 0, 1), *_A(0, 0, 1), ("u", 0, 0, -1), ("u", 0, 0, 0), ("u", 0, 0, 1), ("az_fc", 0, 0, 0))
STENCIL_V = (*_Z(0, 0), *_Z(1, 0), *_Q(0, -1), *_Q(1, -1), *_Q(0, 0), *_Q(1, 0), ("dy_cf", 0, 0, 0), *_K(0, 0), *_K(0, -1),
             *_A(0, -1, 0), *_A(0, 0, 0), *_A(0, -1, 1), *_A(0, 0, 1), ("v", 0, 0, -1), ("v", 0, 0, 0), ("v", 0, 0, 1), ("az_cf", 0, 0, 0))
STENCIL = tuple(sorted(set(STENCIL_U) | set(STENCIL_V)))


def _win(p, size, halo, di=0, dj=0, dk=0, nz=None):
    """the cells (i + di, j + dj, k + dk) for i = 1..Nx, j = 1..Ny, k = 1..nz (default Nz) of a padded parent ((i + di, j + dj) of a plane)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    nz = Nz if nz is None else nz
    ys, xs = slice(Hy + dj, Hy + dj + Ny), slice(Hx + di, Hx + di + Nx)
    return p[ys, xs] if p.ndim == 2 else p[Hz + dk:Hz + dk + nz, ys, xs]


def _check(u, v, w, m, dz_f, size, halo):
    T = u.dtype
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert all(a.dtype == T for a in (v, w, dz_f, *(m[k] for k in METRICS)))
    assert min(halo) >= 1 and dz_f.shape == (Nz + 1,) and u.shape == v.shape == (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    assert w.shape == (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx) and all(m[k].shape == u.shape[1:] for k in METRICS)
    return T


def terms(u, v, w, m, dz_f, size, halo):
    """{"hu", "vu", "bu", "hv", "vv", "bv", "Gu", "Gv"} on the interior, each (Nz, Ny, Nx), in the dtype of u, unmasked; `m` maps the eight
    metric names to their planes"""
    T = _check(u, v, w, m, dz_f, size, halo)
    (Nx, Ny, Nz), _ = size, halo
    half = T.type(0.5)
    W = lambda p, di=0, dj=0, dk=0, nz=None: _win(p, size, halo, di, dj, dk, nz)                                               # noqa: E731
    with np.errstate(all="ignore"):
        Z = lambda di, dj: (((W(m["dy_cf"], di, dj) * W(v, di, dj) - W(m["dy_cf"], di - 1, dj) * W(v, di - 1, dj))             # noqa: E731
                             - (W(m["dx_fc"], di, dj) * W(u, di, dj) - W(m["dx_fc"], di, dj - 1) * W(u, di, dj - 1))) / W(m["az_ff"], di, dj))
        P = lambda di, dj: W(m["dx_cf"], di, dj) * W(v, di, dj)                                                                # noqa: E731
        Q = lambda di, dj: W(m["dy_fc"], di, dj) * W(u, di, dj)                                                                # noqa: E731
        A = lambda di, dj: W(m["az_cc"], di, dj) * W(w, di, dj, 0, Nz + 1)              # faces 1..Nz+1                          # noqa: E731
        K = lambda di, dj: half * (half * (W(u, di, dj) * W(u, di, dj) + W(u, di + 1, dj) * W(u, di + 1, dj))                  # noqa: E731
                                   + half * (W(v, di, dj) * W(v, di, dj) + W(v, di, dj + 1) * W(v, di, dj + 1)))
        d = dz_f[:, None, None]
        zb = half * (Z(0, 0) + Z(0, 1))
        vh = half * (half * (P(-1, 0) + P(-1, 1)) + half * (P(0, 0) + P(0, 1)))
        hu = -((zb * vh) / W(m["dx_fc"]))
        bu = (K(0, 0) - K(-1, 0)) / W(m["dx_fc"])
        S = (half * (A(-1, 0) + A(0, 0))) * ((W(u, 0, 0, 0, Nz + 1) - W(u, 0, 0, -1, Nz + 1)) / d)
        vu = (half * (S[:-1] + S[1:])) / W(m["az_fc"])
        Gu = -((hu + vu) + bu)
        zb = half * (Z(0, 0) + Z(1, 0))
        uh = half * (half * (Q(0, -1) + Q(1, -1)) + half * (Q(0, 0) + Q(1, 0)))
        hv = (zb * uh) / W(m["dy_cf"])
        bv = (K(0, 0) - K(0, -1)) / W(m["dy_cf"])
        R = (half * (A(0, -1) + A(0, 0))) * ((W(v, 0, 0, 0, Nz + 1) - W(v, 0, 0, -1, Nz + 1)) / d)
        vv = (half * (R[:-1] + R[1:])) / W(m["az_cf"])
        Gv = -((hv + vv) + bv)
    out = {"hu": hu, "vu": vu, "bu": bu, "hv": hv, "vv": vv, "bv": bv, "Gu": Gu, "Gv": Gv}
    assert all(a.dtype == T and a.shape == (Nz, Ny, Nx) for a in out.values())
    return out


def zeta(u, v, m, size, halo):
    """the rule's Z on the interior nodes, (Nz, Ny, Nx): the first vorticity of both zb"""
    T = u.dtype
    W = lambda p, di=0, dj=0: _win(p, size, halo, di, dj)                                                                      # noqa: E731
    with np.errstate(all="ignore"):
        z = ((W(m["dy_cf"]) * W(v) - W(m["dy_cf"], -1, 0) * W(v, -1, 0)) - (W(m["dx_fc"]) * W(u) - W(m["dx_fc"], 0, -1) * W(u, 0, -1))) / W(m["az_ff"])
    assert z.dtype == T
    return z


def interior_tendencies(u, v, w, m, dz_f, size, halo):
    """(Gu, Gv) on the interior, each (Nz, Ny, Nx), in the dtype of u, unmasked"""
    t = terms(u, v, w, m, dz_f, size, halo)
    return t["Gu"], t["Gv"]


def tendencies(u, v, w, Gu0, Gv0, m, dz_f, size, halo, n_fc=None, n_cf=None, mask_value=0.0):
    """the parents of (Gu, Gv) after the call: copies of `Gu0`, `Gv0` with the interior replaced, halo cells untouched"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert (n_fc is None) == (n_cf is None)
    out = []
    for G, G0, n in zip(interior_tendencies(u, v, w, m, dz_f, size, halo), (Gu0, Gv0), (n_fc, n_cf)):
        if n is not None:
            assert n.shape == (Ny, Nx)
            k = np.arange(1, Nz + 1)[:, None, None]
            G = np.where(k <= np.minimum(np.maximum(n.astype(np.int64), 0), Nz)[None], u.dtype.type(mask_value), G)
        assert G0.shape == u.shape
        o = G0.copy()
        o[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = G
        out.append(o)
    return tuple(out)


def cells_read(size, halo, stencil=STENCIL):
    """boolean masks of the cells the rule reads, derived from STENCIL: {"u", "v": parent-shaped; "w": its own longer parent; the eight
    metric names: plane-shaped}"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    plane, parent = (Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    read = {"u": np.zeros(parent, bool), "v": np.zeros(parent, bool), "w": np.zeros((Nz + 1 + 2 * Hz,) + plane, bool)}
    read.update({k: np.zeros(plane, bool) for k in METRICS})
    for name, di, dj, dk in stencil:
        _win(read[name], size, halo, di, dj, dk)[...] = True
    return read
