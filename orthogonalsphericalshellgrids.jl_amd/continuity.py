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
from ._operator_plan import OperatorPlan, _check_fields, _ptr, _remembering_field
from .boundary_conditions import Center, Face
from .fields import Field
from .reductions import _bare, _grid_table, _metric, z_center_spacings

_LOCS = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face), "div": (Center, Center, Center)}


def _check(u, v, w, div, what="continuity"):
    _check_fields({"u": (u, _LOCS["u"]), "v": (v, _LOCS["v"]), "w": (w, _LOCS["w"]), "div": (div, _LOCS["div"])}, what, "u, v, w and div",
                  optional=("w", "div"))


class ContinuityPlan(OperatorPlan):
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
            dz = _grid_table(g, "_z_center_spacings", z_center_spacings, dtype, device)
        held = [u.data, v.data, None if w is None else w.data, None if div is None else div.data, dy, dx, az, dz, ncc]
        args = (*(_ptr(t) for t in held), 0.0, u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz, _lib.ft_of(dtype))
        self._set_call(lib.tpg_w_from_continuity, args, _lib.check_continuity, device, held, (w, div) if fill_halos else ())


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
    return _remembering_field(_LOCS["div"], u.grid, "div",
                              lambda twin: ContinuityPlan(u, v, None, twin, fill_halos=fill_halos, mask_immersed=mask_immersed))
