"""Host reference of w from continuity and the horizontal divergence in numpy, on padded parents.

The rule [recalled: Oceananigans' `div_xyᶜᶜᶜ` and `_compute_w_from_continuity!`; parity unpinned, like every operator here.]

Fields
- `u` at (Face, Center, Center) and `v` at (Center, Face, Center): padded parents of geometry `(Nx, Ny, Nz, Hx, Hy, Hz)`.
- `w` at (Center, Center, Face): a padded parent with `Nz + 1` interior levels, `Nz + 1 + 2Hz` planes, same `sx`, `sy`.
- `div` at (Center, Center, Center): a parent like u's.
Metrics
- The grid's padded planes `dy_fc` (`Δyᶠᶜᵃ`), `dx_cf` (`Δxᶜᶠᵃ`), `az_cc` (`Azᶜᶜᵃ`), halos built.
- `dz_c`: `Nz` values `Δzᵃᵃᶜ[k]` in the field type.
Arithmetic, for every interior column `i = 1..Nx`, `j = 1..Ny`, in the field type, in exactly this order, no contraction, every operation one
correctly rounded IEEE operation:
    w[i,j,1] = +0
    for k = 1..Nz, d = dz_c[k]:
        fe = (dy_fc[i+1,j] * d) * u[i+1,j,k]        fw = (dy_fc[i,j] * d) * u[i,j,k]
        fn = (dx_cf[i,j+1] * d) * v[i,j+1,k]        fs = (dx_cf[i,j] * d) * v[i,j,k]
        V  = az_cc[i,j] * d
        div[i,j,k] = (1 / V) * ((fe - fw) + (fn - fs))
        w[i,j,k+1] = w[i,j,k] - d * div[i,j,k]
- `fe` of column `i` IS `fw` of column `i+1`. `fn` of row `j` IS `fs` of row `j+1`. Each is formed once.
- Cells read: `u[1..Nx+1, 1..Ny, 1..Nz]` and the same cells of `dy_fc`; `v[1..Nx, 1..Ny+1, 1..Nz]` and the same cells of `dx_cf`; `az_cc`
  interior; `dz_c`.
- That is one halo column to the east and one halo row to the north, so `Hx ≥ 1` and `Hy ≥ 1`. The caller has filled the halos of u and v.
- On a latitude band `Ny` is the band's row count and row `Ny+1` the exchanged (or, on the last band, folded) north halo row.
- Only interior cells of `w` (levels `1..Nz+1`) and `div` are written.
- `V = 0` divides by it, as the rule says.

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1], planes [j + Hy - 1, i + Hx - 1].  Every operation is one correctly rounded IEEE operation
of the element type, which numpy's elementwise arithmetic in that dtype is too: the reference is exact, comparisons are bit for bit.
With a (Center, Center) count plane n_cc (Ny, Nx), the scan runs on the unmasked values and, where they are stored, div nodes k <= n and w
faces k <= min(n + 1, Nz) hold the mask value instead (what tpg_mask_immersed_fields leaves on a z-Center and a z-Face field)."""
import numpy as np

from vorticity_ref import same_bits  # noqa: F401  (re-exported: the comparison every test of this operator uses)

# the stencil, derived from the rule above: (array, di, dj) of every cell a column (i, j) reads at each level
STENCIL = (("u", 1, 0), ("dy_fc", 1, 0), ("u", 0, 0), ("dy_fc", 0, 0),
           ("v", 0, 1), ("dx_cf", 0, 1), ("v", 0, 0), ("dx_cf", 0, 0), ("az_cc", 0, 0))


def _win(p, size, halo, di=0, dj=0):
    """the cells (i + di, j + dj) for i = 1..Nx, j = 1..Ny of a padded plane or parent (the Nz interior levels of a parent)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    ys, xs = slice(Hy + dj, Hy + dj + Ny), slice(Hx + di, Hx + di + Nx)
    return p[ys, xs] if p.ndim == 2 else p[Hz:Hz + Nz, ys, xs]


def interior_w_and_divergence(u, v, dy_fc, dx_cf, az_cc, dz_c, size, halo):
    """(w, div) on the interior: (Nz + 1, Ny, Nx) and (Nz, Ny, Nx), in the dtype of u, unmasked"""
    T = u.dtype
    assert v.dtype == T and dy_fc.dtype == T and dx_cf.dtype == T and az_cc.dtype == T and dz_c.dtype == T
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert dz_c.shape == (Nz,)
    win = lambda p, di=0, dj=0: _win(p, size, halo, di, dj)
    w = np.zeros((Nz + 1, Ny, Nx), T)                              # w[0] = +0
    div = np.empty((Nz, Ny, Nx), T)
    with np.errstate(all="ignore"):
        for k in range(Nz):
            d = dz_c[k]
            # the fluxes through the Nx + 1 x-faces and the Ny + 1 y-faces of the interior, each formed once
            fx = (dy_fc[Hy:Hy + Ny, Hx:Hx + Nx + 1] * d) * u[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx + 1]
            fy = (dx_cf[Hy:Hy + Ny + 1, Hx:Hx + Nx] * d) * v[Hz + k, Hy:Hy + Ny + 1, Hx:Hx + Nx]
            V = win(az_cc) * d
            div[k] = (T.type(1) / V) * ((fx[:, 1:] - fx[:, :-1]) + (fy[1:, :] - fy[:-1, :]))
            w[k + 1] = w[k] - d * div[k]
    assert w.dtype == T and div.dtype == T
    return w, div


def w_and_divergence(u, v, w0, div0, dy_fc, dx_cf, az_cc, dz_c, size, halo, n_cc=None, mask_value=0.0):
    """the parents of w and div after the call: copies of `w0` and `div0` (either may be None -> None) with the interior replaced, halo cells
    untouched"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    w, div = interior_w_and_divergence(u, v, dy_fc, dx_cf, az_cc, dz_c, size, halo)
    if n_cc is not None:
        mv = u.dtype.type(mask_value)
        k = np.arange(1, Nz + 1)[:, None, None]
        div = np.where(k <= n_cc[None], mv, div)
        kf = np.arange(1, Nz + 2)[:, None, None]
        w = np.where(kf <= np.minimum(n_cc.astype(np.int64) + 1, Nz)[None], mv, w)
    wout = dout = None
    if w0 is not None:
        assert w0.shape == (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
        wout = w0.copy()
        wout[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx] = w
    if div0 is not None:
        assert div0.shape == u.shape
        dout = div0.copy()
        dout[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = div
    return wout, dout


def cells_read(size, halo):
    """boolean masks of the cells the rule reads, derived from STENCIL: {"u", "v": parent-shaped; "dy_fc", "dx_cf", "az_cc": plane-shaped}"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    plane, parent = (Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    read = {"u": np.zeros(parent, bool), "v": np.zeros(parent, bool),
            "dy_fc": np.zeros(plane, bool), "dx_cf": np.zeros(plane, bool), "az_cc": np.zeros(plane, bool)}
    for name, di, dj in STENCIL:
        _win(read[name], size, halo, di, dj)[...] = True
    return read
