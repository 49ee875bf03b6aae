"""Diagnostic operators on a TripolarGrid: the vertical vorticity ζ at (Face, Face, Center), which both of the reference's model drivers
create with VerticalVorticityField(model) and write beside the velocities and tracers on every output (examples/bickley_jet.jl:57,79;
examples/distributed_bickley_jet.jl:59,83).

Everything numeric is tpg_vertical_vorticity (include/tripolar_hip_operators.h, libtripolar_hip_operators.so): one launch over the interior, in the fields' type,
    ζ[i,j,k] = ((Δyᶜᶠᵃ[i,j] v[i,j,k] - Δyᶜᶠᵃ[i-1,j] v[i-1,j,k]) - (Δxᶠᶜᵃ[i,j] u[i,j,k] - Δxᶠᶜᵃ[i,j-1] u[i,j-1,k])) / Azᶠᶠᵃ[i,j]
[recalled: Oceananigans' ζ₃ᶠᶠᶜ; parity unpinned], followed by ζ's own halo fill (the Face-Face fold, sign +1) through the plan machinery of
fields.py.  The halos of u and v are the caller's to fill first, as for any stencil.  On an ImmersedBoundaryGrid the peripheral ζ nodes get 0
inside the same launch (the underlying grid's operator runs on the wet nodes: Oceananigans' conditional differences beside an inactive
velocity node are out of scope).  The plan form holds its tensors: calling it enqueues on torch's current stream and
allocates nothing (usable inside torch.cuda.graph)."""
import torch

from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _ptr, _remembering_field
from .boundary_conditions import Center, Face
from .fields import Field
from .reductions import _bare, _metric

_LOCS = {"u": (Face, Center, Center), "v": (Center, Face, Center), "zeta": (Face, Face, Center)}


def _check(u, v, zeta):
    _check_fields({"u": (u, _LOCS["u"]), "v": (v, _LOCS["v"]), "zeta": (zeta, _LOCS["zeta"])}, "vertical_vorticity", "u, v and zeta",
                  optional=("zeta",))


class VorticityPlan(OperatorPlan):
    """vertical_vorticity(u, v, out=zeta) with its arguments built once: `plan()` issues one tpg_vertical_vorticity call and, with
    `fill_halos`, ζ's halo fill (a HaloFillPlan of zeta) on torch's current stream; it allocates nothing and is a single chain of launches,
    so it replays inside torch.cuda.graph (serial grids: a seam exchange cannot be captured).  On an ImmersedBoundaryGrid with
    `mask_immersed` the (Face, Face) count plane and the value 0 go into the call.  The plan holds the tensors of u, v and zeta, the metric
    arrays and the count plane: rebuild it if a field's `data` is replaced."""

    def __init__(self, u, v, zeta, *, fill_halos=True, mask_immersed=True):
        if zeta is None:
            raise TypeError("vertical_vorticity: zeta must be a Field at (Face, Face, Center)")
        _check(u, v, zeta)
        self.u, self.v, self.zeta = u, v, zeta
        g = _bare(u.grid)
        dtype, device = u.data.dtype, u.data.device
        lib = _lib.operators_lib()
        counts = getattr(u.grid, "column_counts", None) if mask_immersed else None
        nff = None if counts is None else counts["ff"]
        with torch.cuda.device(device):
            dx, dy, az = (_metric(g, name, dtype, device) for name in ("dx_fc", "dy_cf", "az_ff"))
        held = [u.data, v.data, zeta.data, dx, dy, az, nff]
        args = (*(_ptr(t) for t in held), 0.0, u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz, _lib.ft_of(dtype))
        self._set_call(lib.tpg_vertical_vorticity, args, _lib.check_operators, device, held, [zeta] if fill_halos else ())

    def __call__(self):
        super().__call__()
        return self.zeta


def vorticity_plan(u, v, zeta, *, fill_halos=True, mask_immersed=True):
    return VorticityPlan(u, v, zeta, fill_halos=fill_halos, mask_immersed=mask_immersed)


def vertical_vorticity(u, v, out=None, *, fill_halos=True, mask_immersed=True):
    """The vertical vorticity of (u, v) as a Field at (Face, Face, Center): the rule of tpg_vertical_vorticity on every interior node, then
    (with `fill_halos`) the field's own halo fill.  u at (Face, Center, Center) and v at (Center, Face, Center) live on one TripolarGrid,
    share element type and device, and HAVE THEIR HALOS FILLED (the rule reads u[i, j-1] and v[i-1, j]).  `out`: a (Face, Face, Center)
    Field of the same grid to write into; None allocates one with the default conditions (north: Zipper, sign +1).  On an
    ImmersedBoundaryGrid with `mask_immersed` the peripheral ζ nodes are 0, as mask_immersed_field(ζ) would leave them.  z-windowed and
    reduced fields are refused.  Builds a VorticityPlan and runs it once; use vorticity_plan for a field computed on every output."""
    _check(u, v, out)
    zeta = Field(_LOCS["zeta"], u.grid, name="zeta") if out is None else out
    return VorticityPlan(u, v, zeta, fill_halos=fill_halos, mask_immersed=mask_immersed)()


def VerticalVorticityField(u, v, *, fill_halos=True, mask_immersed=True):
    """VerticalVorticityField(model) of the reference's drivers, from the model's velocities: a (Face, Face, Center) Field that remembers
    how it is computed.  Nothing is computed here (the field holds zeros): compute_(field) runs the plan.  The plan works on a second Field
    object over the same tensor, so that the returned field and its plan form no reference cycle (a cycle would keep a multi-GB tensor
    alive until the cycle collector runs)."""
    _check(u, v, None)
    return _remembering_field(_LOCS["zeta"], u.grid, "zeta",
                              lambda twin: VorticityPlan(u, v, twin, fill_halos=fill_halos, mask_immersed=mask_immersed))


def compute_(field):
    """compute!(field): re-run the plan of a field made by VerticalVorticityField; returns the field"""
    plan = getattr(field, "operand_plan", None)
    if plan is None:
        raise TypeError("compute_: the field was not made by VerticalVorticityField (it has no plan to run)")
    plan()
    return field
