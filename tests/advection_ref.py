"""Host reference of the flux-form advection tendency of a tracer in numpy, on padded parents.

The rule [recalled: Oceananigans' div_Uc with Centered(order = 2) in all three directions, _advective_tracer_flux_x/y/z, and
hydrostatic_free_surface_tracer_tendency with no diffusion and no forcing; parity unpinned, like every operator here]

The rule covers every interior node i = 1..Nx, j = 1..Ny, k = 1..Nz.  It is evaluated in the field type T, in exactly this order, with no
contraction.  Every operation is one correctly rounded IEEE operation.
    d = dz_c[k]
    Mx[i,j,k] = (dy_fc[i,j] * d) * u[i,j,k]           i = 1..Nx+1     (the continuity's fe / fw, the same bits)
    My[i,j,k] = (dx_cf[i,j] * d) * v[i,j,k]           j = 1..Ny+1
    Mz[i,j,k] =  az_cc[i,j]      * w[i,j,k]           k = 1..Nz+1     (w has Nz+1 levels)
    Fx[i,j,k] = Mx[i,j,k] * (T(0.5) * (c[i-1,j,k] + c[i,j,k]))
    Fy[i,j,k] = My[i,j,k] * (T(0.5) * (c[i,j-1,k] + c[i,j,k]))
    Fz[i,j,k] = Mz[i,j,k] * (T(0.5) * (c[i,j,k-1] + c[i,j,k]))
    V = az_cc[i,j] * d
    G[i,j,k] = -((T(1) / V) * (((Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])) + (Fz[i,j,k+1] - Fz[i,j,k])))
- Each flux is formed once.  The leading minus is a sign flip.  V = 0 divides by it, as the rule says.
- Cells read: c[0..Nx+1, j, k], c[i, 0..Ny+1, k] and c[i, j, 0..Nz+1] (a plus-shaped stencil, so no corner halo cell); u[1..Nx+1, j, k],
  v[i, 1..Ny+1, k], w[i, j, 1..Nz+1]; the same cells of dy_fc and dx_cf; the interior of az_cc; dz_c.  So Hx, Hy, Hz >= 1.
- Only interior cells of G are written.
- Mask: with a (Center, Center) count plane n_cc (Ny, Nx), the nodes k <= min(max(n, 0), Nz) of G hold T(mask_value) instead; everything is
  computed unmasked (what tpg_mask_immersed_fields leaves on a Center field).

Parents are indexed [k + Hz - 1, j + Hy - 1, i + Hx - 1], planes [j + Hy - 1, i + Hx - 1]; w's parent has Nz + 1 + 2 Hz planes.  Every
operation is one correctly rounded IEEE operation of the element type, which numpy's elementwise arithmetic in that dtype is too: the
reference is exact, comparisons are bit for bit."""
import numpy as np

from vorticity_ref import same_bits  # noqa: F401  (re-exported: the comparison every test of this operator uses)

# the stencil, derived from the rule above: (array, di, dj, dk) of every cell a node (i, j, k) reads
STENCIL = (("c", 0, 0, 0), ("c", -1, 0, 0), ("c", 1, 0, 0), ("c", 0, -1, 0), ("c", 0, 1, 0), ("c", 0, 0, -1), ("c", 0, 0, 1),
           ("u", 0, 0, 0), ("u", 1, 0, 0), ("dy_fc", 0, 0, 0), ("dy_fc", 1, 0, 0),
           ("v", 0, 0, 0), ("v", 0, 1, 0), ("dx_cf", 0, 0, 0), ("dx_cf", 0, 1, 0),
           ("w", 0, 0, 0), ("w", 0, 0, 1), ("az_cc", 0, 0, 0))


def _win(p, size, halo, di=0, dj=0, dk=0):
    """the cells (i + di, j + dj, k + dk) for i = 1..Nx, j = 1..Ny, k = 1..Nz of a padded parent ((i + di, j + dj) of a plane)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    ys, xs = slice(Hy + dj, Hy + dj + Ny), slice(Hx + di, Hx + di + Nx)
    return p[ys, xs] if p.ndim == 2 else p[Hz + dk:Hz + dk + Nz, ys, xs]


def interior_tendency(c, u, v, w, dy_fc, dx_cf, az_cc, dz_c, size, halo):
    """G on the interior, (Nz, Ny, Nx), in the dtype of c, unmasked"""
    T = c.dtype
    assert all(a.dtype == T for a in (u, v, w, dy_fc, dx_cf, az_cc, dz_c))
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert min(halo) >= 1 and dz_c.shape == (Nz,) and c.shape == u.shape == v.shape == (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    assert w.shape == (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    half, one = T.type(0.5), T.type(1)
    ys, xs, zs = slice(Hy, Hy + Ny), slice(Hx, Hx + Nx), slice(Hz, Hz + Nz)
    with np.errstate(all="ignore"):
        d = dz_c[:, None, None]
        # the fluxes through the Nx + 1 x-faces, the Ny + 1 y-faces and the Nz + 1 z-faces of the interior, each formed once
        Mx = (dy_fc[None, ys, Hx:Hx + Nx + 1] * d) * u[zs, ys, Hx:Hx + Nx + 1]
        My = (dx_cf[None, Hy:Hy + Ny + 1, xs] * d) * v[zs, Hy:Hy + Ny + 1, xs]
        Mz = az_cc[None, ys, xs] * w[Hz:Hz + Nz + 1, ys, xs]
        Fx = Mx * (half * (c[zs, ys, Hx - 1:Hx + Nx] + c[zs, ys, Hx:Hx + Nx + 1]))
        Fy = My * (half * (c[zs, Hy - 1:Hy + Ny, xs] + c[zs, Hy:Hy + Ny + 1, xs]))
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
        _win(read[name], size, halo, di, dj, dk)[...] = True
    return read
