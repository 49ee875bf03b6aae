"""The numpy statement of the rule of csrc/staged/tripolar_hip_mixing.h: the convective-adjustment and Ri-based vertical mixing
diffusivities, one IEEE operation per step in the element type T (every array and scalar below has dtype T, so numpy rounds each operation
once, to T).  Held to properties in tests/test_mixing_ref.py; the GPU tests compare to it bit for bit on whole parents.

A problem is a dict: closure ("ca" or "ri"), size, halo, b (u, v for "ri"), dz_f (Nz + 1 values), params (a dict), prev (None or
(kappa_c_prev, nu_c_prev)), counts ({"cc": plane or None, "fc": ..., "cf": ...}), mask_value, outputs (the names wanted, of OUTPUTS).
reference(p, into) returns {name: parent} for the outputs wanted, written into copies of `into[name]` (sentinel-filled parents Face in z)."""
import numpy as np

OUTPUTS = ("kappa_c", "nu_c", "kappa_u", "kappa_v")
COUNT_OF = {"kappa_c": "cc", "nu_c": "cc", "kappa_u": "fc", "kappa_v": "cf"}
CA_PARAMS = ("background_kappa", "convective_kappa", "background_nu", "convective_nu")
RI_PARAMS = ("nu0", "kappa0", "kappa_ca", "Ri0", "Ri_delta", "Cav")


def problem(closure, size, halo, b, dz_f, params, *, u=None, v=None, prev=None, counts=None, mask_value=0.0, outputs=OUTPUTS):
    assert closure in ("ca", "ri") and tuple(params) == (CA_PARAMS if closure == "ca" else RI_PARAMS)
    counts = dict({"cc": None, "fc": None, "cf": None}, **(counts or {}))
    return dict(closure=closure, size=tuple(size), halo=tuple(halo), b=b, u=u, v=v, dz_f=dz_f, params=dict(params), prev=prev, counts=counts,
                mask_value=mask_value, outputs=tuple(outputs))


def cell_shape(size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)


def face_shape(size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)


def taper(Ri, Ri0, Ri_delta):
    """tau of the piecewise-linear taper, in Ri's type: the selects as the header writes them"""
    T = Ri.dtype.type
    with np.errstate(all="ignore"):
        x = (Ri - T(Ri0)) / T(Ri_delta)
        y = np.where(x > 0, x, T(0))
        z = np.where(y < T(1), y, T(1))
        return T(1) - z


def richardson(N2, S2):
    with np.errstate(all="ignore"):
        return np.where(N2 == 0, N2.dtype.type(0), N2 / S2)


def columns(p, di, dj, which):
    """(nu_c, kappa) of the columns (i + di, j + dj) of the interior columns (i, j), at the faces 2..Nz: arrays (Nz - 1, Ny, Nx).  `which`:
    the diffusivities wanted, "nu", "kappa" or both -- what is not wanted is None, and its *_prev array is not touched.  Only the cells the
    header lists are touched"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    T = p["b"].dtype.type
    q = {k: T(x) for k, x in p["params"].items()}
    half, one = T(0.5), T(1)
    dz = np.asarray(p["dz_f"], dtype=T)[1:Nz].reshape(-1, 1, 1)

    def dk(a, si=0, sj=0):                                         # (a[k] - a[k-1]) / dz_f[k] at the columns shifted by (di + si, dj + sj)
        rows = slice(Hy + dj + sj, Hy + dj + sj + Ny)
        cols = slice(Hx + di + si, Hx + di + si + Nx)
        with np.errstate(all="ignore"):
            return (a[Hz + 1:Hz + Nz, rows, cols] - a[Hz:Hz + Nz - 1, rows, cols]) / dz

    def prev(n):
        return p["prev"][n][Hz + 1:Hz + Nz, Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx]

    N2 = dk(p["b"])
    nu = kappa = None
    with np.errstate(all="ignore"):
        if p["closure"] == "ca":
            stable = N2 >= 0
            if "kappa" in which:
                kappa = np.where(stable, q["background_kappa"], q["convective_kappa"])
            if "nu" in which:
                nu = np.where(stable, q["background_nu"], q["convective_nu"])
            return nu, kappa
        du0, du1, dv0, dv1 = dk(p["u"]), dk(p["u"], si=1), dk(p["v"]), dk(p["v"], sj=1)
        su = du0 * du0 + du1 * du1
        sv = dv0 * dv0 + dv1 * dv1
        S2 = half * su + half * sv
        tau = taper(richardson(N2, S2), q["Ri0"], q["Ri_delta"])
        den = one + q["Cav"]
        if "nu" in which:
            nu = q["nu0"] * tau
            if p["prev"] is not None:
                nu = (q["Cav"] * prev(1) + nu) / den
        if "kappa" in which:
            kappa = q["kappa0"] * tau
            kappa = np.where(N2 < 0, kappa + q["kappa_ca"], kappa)
            if p["prev"] is not None:
                kappa = (q["Cav"] * prev(0) + kappa) / den
    return nu, kappa


def richardson_of(p):
    """(N2, S2, Ri) of the interior columns at the faces 2..Nz, by the rule's own operations: arrays (Nz - 1, Ny, Nx)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    T = p["b"].dtype.type
    dz = np.asarray(p["dz_f"], dtype=T)[1:Nz].reshape(-1, 1, 1)

    def dk(a, si=0, sj=0):
        rows, cols = slice(Hy + sj, Hy + sj + Ny), slice(Hx + si, Hx + si + Nx)
        return (a[Hz + 1:Hz + Nz, rows, cols] - a[Hz:Hz + Nz - 1, rows, cols]) / dz
    with np.errstate(all="ignore"):
        N2, du0, du1, dv0, dv1 = dk(p["b"]), dk(p["u"]), dk(p["u"], si=1), dk(p["v"]), dk(p["v"], sj=1)
        S2 = T(0.5) * (du0 * du0 + du1 * du1) + T(0.5) * (dv0 * dv0 + dv1 * dv1)
    return N2, S2, richardson(N2, S2)


def reference(p, into):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    T = p["b"].dtype.type
    half = T(0.5)
    wanted = p["outputs"]
    which = (("kappa",) if "kappa_c" in wanted else ()) + (("nu",) if set(wanted) - {"kappa_c"} else ())
    nu, kappa = columns(p, 0, 0, which)
    values = {"kappa_c": kappa, "nu_c": nu}
    with np.errstate(all="ignore"):
        if "kappa_u" in wanted:
            values["kappa_u"] = half * (columns(p, -1, 0, ("nu",))[0] + nu)
        if "kappa_v" in wanted:
            values["kappa_v"] = half * (columns(p, 0, -1, ("nu",))[0] + nu)
    out = {}
    for name in wanted:
        parent = into[name].copy()
        assert parent.shape == face_shape(p["size"], p["halo"]) and parent.dtype == p["b"].dtype
        faces = np.zeros((Nz + 1, Ny, Nx), T)                       # the faces 1 and Nz + 1 receive T(0)
        faces[1:Nz] = values[name]
        n = p["counts"][COUNT_OF[name]]
        if n is not None:
            k = np.arange(1, Nz + 2).reshape(-1, 1, 1)
            faces = np.where(k <= np.clip(n, 0, Nz)[None] + 1, T(p["mask_value"]), faces)
        parent[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx] = faces
        out[name] = parent
    return out


def cells_read(p):
    """{input name: boolean parent}: the cells the header says are read for p's outputs"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    ri = p["closure"] == "ri"
    wanted = p["outputs"]
    shifts = [(0, 0)] + ([(-1, 0)] if "kappa_u" in wanted else []) + ([(0, -1)] if "kappa_v" in wanted else [])
    read = {"b": np.zeros(cell_shape(p["size"], p["halo"]), bool)}
    if ri:
        read["u"], read["v"] = np.zeros_like(read["b"]), np.zeros_like(read["b"])
        if p["prev"] is not None:
            read["kappa_c_prev"], read["nu_c_prev"] = (np.zeros(face_shape(p["size"], p["halo"]), bool) for _ in range(2))
    if Nz < 2:
        return read
    k = slice(Hz, Hz + Nz)

    def mark(a, di, dj, levels=k):
        a[levels, Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx] = True
    for di, dj in shifts:
        mark(read["b"], di, dj)
        if ri:
            mark(read["u"], di, dj)
            mark(read["u"], di + 1, dj)
            mark(read["v"], di, dj)
            mark(read["v"], di, dj + 1)
    if ri and p["prev"] is not None:
        faces = slice(Hz + 1, Hz + Nz)                             # the faces 2..Nz
        if "kappa_c" in wanted:
            mark(read["kappa_c_prev"], 0, 0, faces)
        if set(wanted) - {"kappa_c"}:
            for di, dj in shifts:
                mark(read["nu_c_prev"], di, dj, faces)
    return read
