"""Host reference of one forward-backward sub-step of the split-explicit free surface in numpy, on padded planes.

The rule [recalled: Oceananigans' `_split_explicit_free_surface!` then `_split_explicit_barotropic_velocity!` on the new eta,
ForwardBackwardScheme; parity unpinned, like every operator here.]

Arrays: eta, U, V, GU, GV, the averages and the five metric planes dy_fc, dx_cf, az_cc, dx_fc, dy_cf are 2-D padded planes of ONE geometry
`(Ny + 2 Hy2) x (Nx + 2 Hx)`, indexed [j + Hy2 - 1, i + Hx - 1]; `depth_of_count`: `Nz + 1` values; n_fc, n_cf: None or (Ny, Nx) int32.
In the field type, in exactly this order, every operation one correctly rounded IEEE operation, dtau, g, weight converted once:
    fe = dy_fc[i+1,j] * U[i+1,j]      fw = dy_fc[i,j] * U[i,j]      fn = dx_cf[i,j+1] * V[i,j+1]      fs = dx_cf[i,j] * V[i,j]
    eta'[i,j] = eta[i,j] - dtau * (((fe - fw) + (fn - fs)) / az_cc[i,j])                                 i = 1..Nx, j = 1..Ny
    U'[i,j] = U[i,j] + dtau * (GU[i,j] - (g * Hfc) * ((eta'[i,j] - eta'[i-1,j]) / dx_fc[i,j]))          eta'[0,j] = eta'[Nx,j]
    V'[i,j] = V[i,j] + dtau * (GV[i,j] - (g * Hcf) * ((eta'[i,j] - eta'[i,j-1]) / dy_cf[i,j]))          j = 2..Ny;  V'[i,1] = V[i,1]
    eta_bar += weight * eta',  U_bar += weight * U',  V_bar += weight * V'
with Hfc = depth_of_count[min(max(n_fc[i,j], 0), Nz)] (None: depth_of_count[0]), Hcf from n_cf.  numpy's elementwise arithmetic in the dtype
is one correctly rounded IEEE operation per operation: the reference is exact, comparisons are bit for bit."""
import numpy as np

from vorticity_ref import same_bits  # noqa: F401  (re-exported: the comparison every test of this pass uses)

METRICS = ("dy_fc", "dx_cf", "az_cc", "dx_fc", "dy_cf")


def _win(p, size, Hx, Hy2, dj=0, di=0):
    """the interior window of a plane, shifted by (dj, di)"""
    Nx, Ny = size[0], size[1]
    assert p.shape == (Ny + 2 * Hy2, Nx + 2 * Hx), (p.shape, size, Hx, Hy2)
    return p[Hy2 + dj:Hy2 + dj + Ny, Hx + di:Hx + di + Nx]


def _depths(depth_of_count, n, size):
    Nx, Ny, Nz = size
    assert depth_of_count.shape == (Nz + 1,)
    idx = np.zeros((Ny, Nx), np.int64) if n is None else np.clip(n.astype(np.int64), 0, Nz)
    return depth_of_count[idx]


def interior_substep(eta, U, V, GU, GV, metrics, depth_of_count, size, Hx, Hy2, dtau, g, n_fc=None, n_cf=None):
    """the interiors (eta', U', V'), each (Ny, Nx) in the dtype of eta; `metrics`: {name: plane} of METRICS"""
    T = eta.dtype
    assert all(a.dtype == T for a in (U, V, GU, GV, depth_of_count, *(metrics[k] for k in METRICS)))
    w = lambda p, dj=0, di=0: _win(p, size, Hx, Hy2, dj, di)
    dtau, g = T.type(dtau), T.type(g)
    with np.errstate(all="ignore"):
        fe, fw = w(metrics["dy_fc"], 0, 1) * w(U, 0, 1), w(metrics["dy_fc"]) * w(U)
        fn, fs = w(metrics["dx_cf"], 1, 0) * w(V, 1, 0), w(metrics["dx_cf"]) * w(V)
        d = ((fe - fw) + (fn - fs)) / w(metrics["az_cc"])
        etap = w(eta) - dtau * d
        west = np.roll(etap, 1, axis=1)                            # eta'[i-1, j]; column 1 takes column Nx: the periodic wrap, recomputed
        px = (etap - west) / w(metrics["dx_fc"])
        Up = w(U) + dtau * (w(GU) - (g * _depths(depth_of_count, n_fc, size)) * px)
        py = (etap[1:] - etap[:-1]) / w(metrics["dy_cf"])[1:]
        Vp = w(V).copy()                                           # row 1 is carried
        Vp[1:] = w(V)[1:] + dtau * (w(GV)[1:] - (g * _depths(depth_of_count, n_cf, size))[1:] * py)
    assert etap.dtype == T and Up.dtype == T and Vp.dtype == T
    return etap, Up, Vp


def substep(out0, state, G, metrics, depth_of_count, size, Hx, Hy2, dtau, g, n_fc=None, n_cf=None, averages=None, weight=0.0):
    """the planes (eta_out, U_out, V_out) after the call -- copies of `out0` with the interior replaced, every other cell untouched -- and the
    averages after it (copies with `weight` times the new interiors added; None without averaging); `state` = (eta, U, V), `G` = (GU, GV)"""
    new = interior_substep(*state, *G, metrics, depth_of_count, size, Hx, Hy2, dtau, g, n_fc, n_cf)
    outs = []
    for p0, x in zip(out0, new):
        p = p0.copy()
        _win(p, size, Hx, Hy2)[...] = x
        outs.append(p)
    if averages is None:
        return tuple(outs), None
    T = state[0].dtype
    bars = []
    for b0, x in zip(averages, new):
        b = b0.copy()
        with np.errstate(all="ignore"):
            _win(b, size, Hx, Hy2)[...] = _win(b0, size, Hx, Hy2) + T.type(weight) * x
        bars.append(b)
    return tuple(outs), tuple(bars)


def cells_read(size, Hx, Hy2, n_fc=None, n_cf=None):
    """boolean masks of the cells the rule reads, by argument name: planes of the padded shape for eta, U, V, GU, GV, the five metrics and
    "average" (the three alike); (Ny, Nx) for n_fc / n_cf; the Nz + 1 entries of depth_of_count some count that is read selects (entry 0
    where a plane is None).  U and dy_fc: the interior and the east halo column Nx + 1; V and dx_cf: the interior and the north halo row
    Ny + 1; GV, dy_cf and n_cf: rows 2..Ny (row 1 of V is carried); everything else: the interior."""
    Nx, Ny, Nz = size
    shape = (Ny + 2 * Hy2, Nx + 2 * Hx)
    inner = np.zeros(shape, bool)
    _win(inner, size, Hx, Hy2)[...] = True
    east, north, upper = inner.copy(), inner.copy(), inner.copy()
    east[Hy2:Hy2 + Ny, Hx + Nx] = True
    north[Hy2 + Ny, Hx:Hx + Nx] = True
    upper[Hy2] = False
    read = {"eta": inner, "U": east, "dy_fc": east, "V": north, "dx_cf": north, "az_cc": inner, "dx_fc": inner, "GU": inner, "GV": upper,
            "dy_cf": upper, "average": inner, "n_fc": np.ones((Ny, Nx), bool), "n_cf": np.ones((Ny, Nx), bool)}
    read["n_cf"][0] = False
    depth = np.zeros(Nz + 1, bool)
    for n, rows in ((n_fc, slice(0, None)), (n_cf, slice(1, None))):
        if n is None:
            depth[0] = True
        else:
            depth[np.clip(n[rows].astype(np.int64), 0, Nz)] = True
    read["depth_of_count"] = depth
    return read
