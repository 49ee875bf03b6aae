"""The rule of tpg_diffusive_tendency (csrc/staged/tripolar_hip_diffusion.h) in numpy, in the field type: the reference the GPU tests compare
with bit for bit, itself held to properties by tests/test_diffusion_ref.py.

Two statements of the one rule: tendency_column, the header's lines word for word on one column with 1-based indices and Python scalars of
the field type, and tendency_planes, the same operations on whole planes at once (what the GPU tests can afford); the property tests require
the two to agree bit for bit.  Neither uses a fused operation: numpy's scalar and array arithmetic rounds every operation once.

Arrays are the padded parents, indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1]; planes [j + Hy - 1, i + Hx - 1]; count planes (Ny, Nx)."""
import numpy as np

HORIZONTAL, VERTICAL = 1, 2
ADD, WRITE = 0, 1
CONSTANT, PROFILE, FIELD = 0, 1, 2


def first_wet(count, Nz):
    """k0 of the header, 1-based"""
    return 1 if count is None else min(max(int(count), 0), Nz) + 1


def vertical_present(terms, top, bottom):
    """the vertical group is a property of the call: the bit, or a flux table (a list, whatever its entries)"""
    return bool(terms & VERTICAL) or top is not None or bottom is not None


def kappa_face(kappa, form, k, j, i, halo, T):
    """kz at the face k (1-based) of the column (i, j) (1-based)"""
    Hx, Hy, Hz = halo
    if form == CONSTANT:
        return T(kappa)
    if form == PROFILE:
        return T(kappa[k - 1])
    return T(kappa[Hz + k - 1, Hy + j - 1, Hx + i - 1])


def tendency_column(p, q, i, j):
    """G[q] of the column (i, j), 1-based, as Nz values: the header's lines on scalars.  p: the problem (see `problem`)."""
    c, T = p["c"][q], p["c"][q].dtype.type
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    terms, top, bottom = p["terms"], p["top"], p["bottom"]
    C = lambda ii, jj, kk: T(c[Hz + kk - 1, Hy + jj - 1, Hx + ii - 1])          # noqa: E731
    P = lambda name, ii, jj: T(p[name][Hy + jj - 1, Hx + ii - 1])               # noqa: E731
    zero = T(0)
    k0 = first_wet(None if p["counts"] is None else p["counts"][j - 1, i - 1], Nz)

    def inactive(ii, jj, kk):
        if p["h"] is None:
            return False
        if jj < 1 and p["wall"]:
            return True
        return bool(T(p["zc"][kk - 1]) <= T(p["h"][Hy + jj - 1, Hx + ii - 1]))

    out = []
    with np.errstate(all="ignore"):
        for k in range(1, Nz + 1):
            d = T(p["dz_c"][k - 1])
            V = P("az", i, j) * d
            S = None
            if terms & HORIZONTAL:
                kh = T(p["kappa_h"])

                def Fx(ii):
                    if inactive(ii - 1, j, k) or inactive(ii, j, k):
                        return zero
                    return (kh * (P("dy_fc", ii, j) * d)) * ((C(ii, j, k) - C(ii - 1, j, k)) / P("dx_fc", ii, j))

                def Fy(jj):
                    if inactive(i, jj - 1, k) or inactive(i, jj, k):
                        return zero
                    return (kh * (P("dx_cf", i, jj) * d)) * ((C(i, jj, k) - C(i, jj - 1, k)) / P("dy_cf", i, jj))
                S = (Fx(i + 1) - Fx(i)) + (Fy(j + 1) - Fy(j))
            if vertical_present(terms, top, bottom):
                def Fz(kk):
                    if kk == k0:
                        return -(P("az", i, j) * T(bottom[q][Hy + j - 1, Hx + i - 1])) if bottom is not None and bottom[q] is not None else zero
                    if kk == Nz + 1:
                        return -(P("az", i, j) * T(top[q][Hy + j - 1, Hx + i - 1])) if top is not None and top[q] is not None else zero
                    if kk < k0 or not terms & VERTICAL:
                        return zero
                    kz = kappa_face(p["kappa_z"], p["form"], kk, j, i, p["halo"], T)
                    return (kz * P("az", i, j)) * ((C(i, j, kk) - C(i, j, kk - 1)) / T(p["dz_f"][kk - 1]))
                Vsum = Fz(k + 1) - Fz(k)
                S = Vsum if S is None else S + Vsum
            D = (T(1) / V) * S
            if p["mode"] == ADD:
                D = T(p["G"][q][Hz + k - 1, Hy + j - 1, Hx + i - 1]) + D
            out.append(T(p["mask_value"]) if (p["counts"] is not None and k < k0) else D)
    return np.array(out, dtype=T)


def inactive_planes(p, T):
    """inactive(i, j, k) for i = 0..Nx+1, j = 0..Ny+1, k = 1..Nz, indexed [k-1, j, i]; all False without a bottom height"""
    (Nx, Ny, Nz), (Hx, Hy, _) = p["size"], p["halo"]
    ina = np.zeros((Nz, Ny + 2, Nx + 2), dtype=bool)
    if p["h"] is not None:
        h = np.asarray(p["h"], dtype=T)[Hy - 1:Hy + Ny + 1, Hx - 1:Hx + Nx + 1]
        ina[...] = np.asarray(p["zc"], dtype=T)[:, None, None] <= h[None]
        if p["wall"]:
            ina[:, 0, :] = True
    return ina


def closed_faces(p, T):
    """(closed_x for i = 1..Nx+1, closed_y for j = 1..Ny+1) of the interior rows / columns, indexed [k-1, j-1, i-1]"""
    (Nx, Ny, _) = p["size"]
    ina = inactive_planes(p, T)
    return ina[:, 1:Ny + 1, 0:Nx + 1] | ina[:, 1:Ny + 1, 1:Nx + 2], ina[:, 0:Ny + 1, 1:Nx + 1] | ina[:, 1:Ny + 2, 1:Nx + 1]


def tendency_planes(p, q, fluxes=None):
    """G[q] of the whole interior, (Nz, Ny, Nx): the same operations on arrays.  `fluxes`: a dict that receives Fx (Nz, Ny, Nx + 1), Fy
    (Nz, Ny + 1, Nx) and Fz (Nz + 1, Ny, Nx) of the groups that are present"""
    c, T = p["c"][q], p["c"][q].dtype.type
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    terms, top, bottom = p["terms"], p["top"], p["bottom"]
    ys, xs = slice(Hy, Hy + Ny), slice(Hx, Hx + Nx)
    zero = T(0)
    dz_c = np.asarray(p["dz_c"], dtype=T)
    d = dz_c[:, None, None]
    az = p["az"][ys, xs]
    m = np.zeros((Ny, Nx), dtype=np.int64) if p["counts"] is None else np.clip(np.asarray(p["counts"], dtype=np.int64), 0, Nz)
    S = None
    with np.errstate(all="ignore"):
        V = az[None] * d
        if terms & HORIZONTAL:
            kh = T(p["kappa_h"])
            cx, cy = closed_faces(p, T)
            ci = c[Hz:Hz + Nz]
            Fx = (kh * (p["dy_fc"][ys, Hx:Hx + Nx + 1][None] * d)) * ((ci[:, ys, Hx:Hx + Nx + 1] - ci[:, ys, Hx - 1:Hx + Nx]) / p["dx_fc"][ys, Hx:Hx + Nx + 1][None])
            Fy = (kh * (p["dx_cf"][Hy:Hy + Ny + 1, xs][None] * d)) * ((ci[:, Hy:Hy + Ny + 1, xs] - ci[:, Hy - 1:Hy + Ny, xs]) / p["dy_cf"][Hy:Hy + Ny + 1, xs][None])
            Fx, Fy = np.where(cx, zero, Fx), np.where(cy, zero, Fy)
            S = (Fx[:, :, 1:] - Fx[:, :, :-1]) + (Fy[:, 1:] - Fy[:, :-1])
            if fluxes is not None:
                fluxes.update(Fx=Fx, Fy=Fy)
        if vertical_present(terms, top, bottom):
            ci = c[Hz:Hz + Nz, ys, xs]
            Fz = np.zeros((Nz + 1, Ny, Nx), dtype=T)               # 0-based face k lies under cell k
            if terms & VERTICAL and Nz > 1:
                form, kap = p["form"], p["kappa_z"]
                if form == CONSTANT:
                    kz = np.full((Nz - 1, 1, 1), T(kap), dtype=T)
                elif form == PROFILE:
                    kz = np.asarray(kap, dtype=T)[1:Nz, None, None]
                else:
                    kz = kap[Hz + 1:Hz + Nz, ys, xs]
                dz_f = np.asarray(p["dz_f"], dtype=T)[1:Nz, None, None]
                Fz[1:Nz] = (kz * az[None]) * ((ci[1:] - ci[:-1]) / dz_f)
            k = np.arange(Nz + 1)[:, None, None]
            Fb = -(az * bottom[q][ys, xs]) if bottom is not None and bottom[q] is not None else np.zeros((Ny, Nx), dtype=T)
            Ft = -(az * top[q][ys, xs]) if top is not None and top[q] is not None else np.zeros((Ny, Nx), dtype=T)
            Fz = np.where(k <= m[None], Fb[None], Fz)              # the face under the lowest wet cell (below it: masked cells)
            Fz[Nz] = Ft
            Vsum = Fz[1:] - Fz[:-1]
            if fluxes is not None:
                fluxes.update(Fz=Fz)
            S = Vsum if S is None else S + Vsum
        D = (T(1) / V) * S
        if p["mode"] == ADD:
            D = p["G"][q][Hz:Hz + Nz, ys, xs] + D
    if p["counts"] is not None:
        D = np.where(np.arange(Nz)[:, None, None] < m[None], T(p["mask_value"]), D)
    assert D.dtype == c.dtype
    return D


def problem(c, G, terms, mode, size, halo, *, az, dz_c, kappa_h=0.0, kappa_z=0.0, form=CONSTANT, dz_f=None, top=None, bottom=None, dx_fc=None,
            dy_fc=None, dx_cf=None, dy_cf=None, counts=None, mask_value=0.0, h=None, zc=None, wall=True):
    """the arguments of one call, by the header's names: c, G lists of padded parents; top, bottom None or lists of None / padded planes"""
    return dict(c=list(c), G=list(G), terms=terms, mode=mode, size=tuple(size), halo=tuple(halo), az=az, dz_c=dz_c, kappa_h=kappa_h, kappa_z=kappa_z,
                form=form, dz_f=dz_f, top=top, bottom=bottom, dx_fc=dx_fc, dy_fc=dy_fc, dx_cf=dx_cf, dy_cf=dy_cf, counts=counts, mask_value=mask_value,
                h=h, zc=zc, wall=wall)


def reference(p):
    """what the call leaves in the padded parents G: new arrays, the halos as they were"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    out = []
    for q, g in enumerate(p["G"]):
        new = g.copy()
        new[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = tendency_planes(p, q)
        out.append(new)
    return out


def by_columns(p, q):
    """tendency_column over the whole interior, (Nz, Ny, Nx)"""
    Nx, Ny, Nz = p["size"]
    out = np.empty((Nz, Ny, Nx), dtype=p["c"][q].dtype)
    for j in range(1, Ny + 1):
        for i in range(1, Nx + 1):
            out[:, j - 1, i - 1] = tendency_column(p, q, i, j)
    return out
