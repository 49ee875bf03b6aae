"""w from continuity and the horizontal divergence on a TripolarGrid: what a hydrostatic model diagnoses from u and v after every velocity
update, before its time-step wizard (cell_advection_timescale reads w) and its output writer, which the reference's drivers point at
model.velocities, w included.

Everything numeric is tpg_w_from_continuity (include/tripolar_hip_continuity.h, libtripolar_hip_continuity.so): one launch over the interior
columns, in the fields' type,
    w[i,j,1] = +0
    for k = 1..Nz, d = Δzᵃᵃᶜ[k]:
        fe = (Δyᶠᶜᵃ[i+1,j] d) u[i+1,j,k]      fw = (Δyᶠᶜᵃ[i,j] d) u[i,j,k]      fn = (Δxᶜᶠᵃ[i,j+1] d) v[i,j+1,k]      fs = (Δxᶜᶠᵃ[i,j] d) v[i,j,k]
        div[i,j,k] = (1 / (Azᶜᶜᵃ[i,j] d)) ((fe - fw) + (fn - fs))
        w[i,j,k+1] = w[i,j,k] - d div[i,j,k]
[recalled: Oceananigans' div_xyᶜᶜᶜ and _compute_w_from_continuity!; parity unpinned], followed by the outputs' own halo fill through the plan
machinery of fields.py.  The halos of u and v are the caller's to fill first: column Nx reads u[Nx+1, j], the periodic image, and row Ny reads
v[i, Ny+1], the first row the Zipper fold writes, with its sign flip.  On an ImmersedBoundaryGrid the peripheral nodes of w and div get 0
inside the same launch (the underlying grid's operator runs on every column: Oceananigans' conditional differences beside an inactive
velocity node are out of scope).  The plan form holds its tensors: calling it enqueues on torch's current stream and allocates
nothing (usable inside torch.cuda.graph)."""
import torch

from . import _lib
from .boundary_conditions import Center, Face
from .fields import Field, HaloFillPlan
from .grids import is_tripolar
from .reductions import _bare, _metric

_LOCS = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face), "div": (Center, Center, Center)}


def z_center_spacings(grid, dtype=None):
    """Δzᵃᵃᶜ[k] for k = 1..Nz: the face-to-face spacing at centre k, computed in float64 from grid.z_spec and rounded ONCE to `dtype` (default:
    the grid's), as z_face_spacings is.  A regular interval (z0, z1) gives (z1 - z0) / Nz at every level; explicit faces give the float64
    differences of adjacent faces.  A float64 host tensor of values that are exact in `dtype`."""
    g = _bare(grid)
    Nz = g.Nz
    zz = g.z_spec.flatten().tolist() if torch.is_tensor(g.z_spec) else list(g.z_spec)
    if len(zz) == 2:
        d = torch.full((Nz,), (float(zz[1]) - float(zz[0])) / Nz, dtype=torch.float64)
    else:
        f = torch.tensor([float(z) for z in zz], dtype=torch.float64)
        d = f[1:Nz + 1] - f[0:Nz]
    return d.to(dtype or g.dtype).to(torch.float64)


def _dz_c(grid, dtype, device):
    """the device copy of z_center_spacings, built once per (grid, type) and kept with the grid"""
    g = _bare(grid)
    cache = g.__dict__.setdefault("_z_center_spacings", {})
    key = (dtype, str(device))
    if key not in cache:
        cache[key] = z_center_spacings(g, dtype).to(dtype).to(device)
    return cache[key]


def _check(u, v, w, div, what="continuity"):
    for name, f in (("u", u), ("v", v), ("w", w), ("div", div)):
        if f is None and name in ("w", "div"):
            continue
        loc = _LOCS[name]
        if not isinstance(f, Field) or f.loc != loc:
            raise TypeError(f"{what}: {name} must be a Field at ({', '.join(L.__name__ for L in loc)})")
        if f.grid is not u.grid:
            raise ValueError(f"{what}: u, v, w and div must live on one grid")
        if f.z_window is not None:
            raise NotImplementedError(f"{what}: z-windowed fields are not handled")
        if f.data.dtype != u.data.dtype or f.data.device != u.data.device:
            raise ValueError(f"{what}: u, v, w and div must share one element type and device")
    if not is_tripolar(u.grid):
        raise TypeError(f"{what}: the fields' grid must be a TripolarGrid")


class ContinuityPlan:
    """compute_w_from_continuity(u, v, w) / horizontal_divergence(u, v, out=div) with the arguments built once: `plan()` issues ONE
    tpg_w_from_continuity call on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of the outputs it has -- the outputs'
    own conditions, whatever they are.  An impenetrable (Open) TOP on w would overwrite the computed surface value w[Nz+1]: a free-surface
    model's w has none, and neither has the default ZFaceField.  It allocates nothing and is a single chain of launches, so it replays inside
    torch.cuda.graph (serial grids: a seam exchange cannot be captured).  On an ImmersedBoundaryGrid with `mask_immersed` the
    (Center, Center) count plane and the value 0 go into the call.  The plan holds the tensors of u, v and the outputs, the metric arrays,
    the spacings and the count plane: rebuild it if a field's `data` is replaced."""

    def __init__(self, u, v, w=None, div=None, *, fill_halos=True, mask_immersed=True):
        _check(u, v, w, div)
        if w is None and div is None:
            raise TypeError("continuity: at least one output, w at (Center, Center, Face) or div at (Center, Center, Center), is needed")
        self.u, self.v, self.w, self.div = u, v, w, div
        g = _bare(u.grid)
        dtype, device = u.data.dtype, u.data.device
        lib = _lib.continuity_lib()
        counts = getattr(u.grid, "column_counts", None) if mask_immersed else None
        ncc = None if counts is None else counts["cc"]
        with torch.cuda.device(device):
            dy, dx, az = (_metric(g, name, dtype, device) for name in ("dy_fc", "dx_cf", "az_cc"))
            dz = _dz_c(g, dtype, device)
        wd, dd = (None if f is None else f.data for f in (w, div))
        self._held = [u.data, v.data, wd, dd, dy, dx, az, dz, ncc]
        ptr = lambda t: None if t is None else t.data_ptr()
        args = (u.data.data_ptr(), v.data.data_ptr(), ptr(wd), ptr(dd), dy.data_ptr(), dx.data_ptr(), az.data_ptr(), dz.data_ptr(),
                ptr(ncc), 0.0, u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz, _lib.ft_of(dtype))
        self._device, self._call = device, (lib.tpg_w_from_continuity, args)
        outs = [f for f in (w, div) if f is not None and f.boundary_conditions is not None]
        self._fill = HaloFillPlan(outs) if fill_halos and outs else None

    def __call__(self):
        fn, args = self._call
        with torch.cuda.device(self._device):
            _lib.check_continuity(fn(*args, _lib.current_stream_ptr(self._device)))
        if self._fill is not None:
            self._fill()
        return self


def continuity_plan(u, v, w=None, div=None, *, fill_halos=True, mask_immersed=True):
    return ContinuityPlan(u, v, w, div, fill_halos=fill_halos, mask_immersed=mask_immersed)


def compute_w_from_continuity(u, v, w=None, *, fill_halos=True, mask_immersed=True):
    """w at (Center, Center, Face) from the continuity equation integrated upward from w[1] = +0: the rule of tpg_w_from_continuity on every
    interior column, then (with `fill_halos`) w's own halo fill.  u at (Face, Center, Center) and v at (Center, Face, Center) live on one
    TripolarGrid, share element type and device, and HAVE THEIR HALOS FILLED (the rule reads u[i+1, j] and v[i, j+1]).  `w`: the field to write
    into; None allocates ZFaceField(grid).  Returns w.  Builds a ContinuityPlan and runs it once; use continuity_plan in a time loop."""
    _check(u, v, w, None, "compute_w_from_continuity")
    w = Field(_LOCS["w"], u.grid, name="w") if w is None else w
    ContinuityPlan(u, v, w, None, fill_halos=fill_halos, mask_immersed=mask_immersed)()
    return w


def horizontal_divergence(u, v, out=None, *, fill_halos=True, mask_immersed=True):
    """The horizontal divergence of (u, v) as a Field at (Center, Center, Center): div of the rule of tpg_w_from_continuity (nothing carries
    from level to level), then (with `fill_halos`) the field's own halo fill.  `out`: the field to write into; None allocates
    CenterField(grid).  Returns it."""
    _check(u, v, None, out, "horizontal_divergence")
    div = Field(_LOCS["div"], u.grid, name="div") if out is None else out
    ContinuityPlan(u, v, None, div, fill_halos=fill_halos, mask_immersed=mask_immersed)()
    return div


def HorizontalDivergenceField(u, v, *, fill_halos=True, mask_immersed=True):
    """A (Center, Center, Center) Field that remembers how it is computed from the model's velocities.  Nothing is computed here (the field
    holds zeros): compute_(field) runs the plan.  The plan works on a second Field object over the same tensor, so that the returned field and
    its plan form no reference cycle (a cycle would keep a multi-GB tensor alive until the cycle collector runs)."""
    _check(u, v, None, None, "HorizontalDivergenceField")
    div = Field(_LOCS["div"], u.grid, name="div")
    twin = Field(_LOCS["div"], u.grid, data=div.data, boundary_conditions=div.boundary_conditions, name="div")
    div.operand_plan = ContinuityPlan(u, v, None, twin, fill_halos=fill_halos, mask_immersed=mask_immersed)
    return div
