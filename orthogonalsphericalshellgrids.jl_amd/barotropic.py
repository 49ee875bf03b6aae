"""The two ends of a split-explicit free surface's sub-cycle on a TripolarGrid: the barotropic mode of the 3-D velocities before it and the
velocity correction after it, before w is diagnosed from continuity.  The reference's drivers build
HydrostaticFreeSurfaceModel(; grid, free_surface = SplitExplicitFreeSurface(grid; substeps = 30)) (examples/bickley_jet.jl:44-55); the
sub-cycle between the two calls is free_surface.py's (SplitExplicitFreeSurface, split_explicit_subcycle_plan).

Everything numeric is tpg_barotropic_mode / tpg_barotropic_correction (include/tripolar_hip_barotropic.h, libtripolar_hip_barotropic.so): one
launch each over the interior columns, in the fields' type,
    Ū[i,j] = Δzᵃᵃᶜ[1] u[i,j,1];   for k = 2..Nz:  Ū[i,j] = Ū[i,j] + Δzᵃᵃᶜ[k] u[i,j,k]                       (V̄ from v likewise)
    H = depth_of_count[min(n_fc[i,j], Nz)];   c = (U[i,j] - Ū[i,j]) / H;   u[i,j,k] = u[i,j,k] + c   k = 1..Nz    (v with V, V̄, n_cf)
[recalled: Oceananigans' compute_barotropic_mode! and barotropic_split_explicit_corrector!; parity unpinned], followed by the outputs' own
halo fill through the plan machinery of fields.py.  The 2-D fields may live on another grid object than u and v -- the case that matters is
with_halo((Hx, Hy2, Hz), grid), the extended-halo grid of the free surface (test/runtests.jl:69-71): they share Nx, Ny, Hx, element type and
device with u, and their own north / south halo Hy2 goes into the call.  On an ImmersedBoundaryGrid the correction masks the peripheral nodes
of u and v inside the same launch.  The plan forms hold their tensors: calling one enqueues on torch's current stream and allocates nothing
(usable inside torch.cuda.graph)."""
import torch

from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _ptr, _require
from .boundary_conditions import Center, Face
from .fields import Field
from .grids import is_tripolar
from .reductions import _bare, _grid_table, _z_spec_values, z_center_spacings

_LOCS = {"u": (Face, Center, Center), "v": (Center, Face, Center),
         "U": (Face, Center, None), "V": (Center, Face, None), "Ubar": (Face, Center, None), "Vbar": (Center, Face, None)}


def column_depth_table(grid, dtype=None):
    """depth_of_count[n] for n = 0..Nz: the depth z_face[Nz+1] - z_face[n+1] of a column whose lowest n cells are immersed, computed in
    float64 from the faces of grid.z_spec and rounded ONCE to `dtype` (default: the grid's), as z_center_spacings is.  A regular interval
    (z0, z1) has the faces z0 + (z1 - z0) n / Nz, the last one z1 itself.  A float64 host tensor of Nz + 1 values that are exact in `dtype`;
    the first is the rounded full depth, the last +0.
    [recalled: the static column depth of a grid-fitted bottom snapped to a face; the (Face, Center) count is the max of the two neighbouring
    columns' counts, which gives Oceananigans' min of the two depths.  Parity unpinned, like every operator.]"""
    g = _bare(grid)
    Nz = g.Nz
    zz = _z_spec_values(g)
    if len(zz) == 2:
        z0, z1 = float(zz[0]), float(zz[1])
        faces = [z0 + (z1 - z0) * n / Nz for n in range(Nz)] + [z1]
    else:
        faces = [float(z) for z in zz][:Nz + 1]
    f = torch.tensor(faces, dtype=torch.float64)
    return (f[Nz] - f).to(dtype or g.dtype).to(torch.float64)


def _check(fields, what):
    """`fields`: {name: Field or None} of u, v and the 2-D fields of one call: u and v through the shared checker (each may be None), then
    what only the 2-D planes need -- they may live on another grid, which shares Nx, Ny and Hx with u's, and have one north/south halo."""
    first = _check_fields({n: (fields[n], _LOCS[n]) for n in ("u", "v")}, what, "u and v", optional=("u", "v"),
                          type_group="u, v and the 2-D fields")
    if first is None:
        raise TypeError(f"{what}: at least one of u at (Face, Center, Center) and v at (Center, Face, Center) is needed")
    planes = [(n, fields[n]) for n in ("U", "V", "Ubar", "Vbar") if fields.get(n) is not None]
    for name, f in planes:
        _require(f, name, _LOCS[name], what)
        if not is_tripolar(f.grid):
            raise TypeError(f"{what}: the fields' grid must be a TripolarGrid")
        if (f.Nx, f.Ny, f.Hx) != (first.Nx, first.Ny, first.Hx):
            raise ValueError(f"{what}: {name} must share Nx, Ny and Hx with u and v (size {f.Nx}x{f.Ny}, Hx {f.Hx} against "
                             f"{first.Nx}x{first.Ny}, Hx {first.Hx})")
        if f.Hy != planes[0][1].Hy:
            raise ValueError(f"{what}: the 2-D fields must share one north/south halo (Hy {f.Hy} against {planes[0][1].Hy})")
        if f.data.dtype != first.data.dtype or f.data.device != first.data.device:
            raise ValueError(f"{what}: u, v and the 2-D fields must share one element type and device")
    return first


class BarotropicModePlan(OperatorPlan):
    """compute_barotropic_mode(u, v, U, V) with the arguments built once: `plan()` issues ONE tpg_barotropic_mode call on torch's current
    stream and then, with `fill_halos`, ONE HaloFillPlan of (U, V) -- their own conditions, the sign-flipping zipper into every north halo
    row they have.  It allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  A pair
    (u, U) or (v, V) may be None together; with both of U and V None the plan allocates them beside the 3-D fields it was given, on their
    grid.  The plan holds the tensors of the fields and the spacings: rebuild it if a field's `data` is replaced."""

    def __init__(self, u, v, U=None, V=None, *, fill_halos=True, what="barotropic_mode_plan"):
        first = _check({"u": u, "v": v, "U": U, "V": V}, what)
        if U is None and V is None:
            U = None if u is None else Field(_LOCS["U"], u.grid, name="U")
            V = None if v is None else Field(_LOCS["V"], v.grid, name="V")
        if (u is None) != (U is None) or (v is None) != (V is None):
            raise TypeError(f"{what}: u and U, and v and V, are given together (a pair may be None together; both of U and V None allocates them)")
        self.u, self.v, self.U, self.V = u, v, U, V
        g = _bare(first.grid)
        dtype, device = first.data.dtype, first.data.device
        lib = _lib.barotropic_lib()
        with torch.cuda.device(device):
            dz = _grid_table(g, "_z_center_spacings", z_center_spacings, dtype, device)
        held = [f.data for f in (u, v, U, V) if f is not None] + [dz]
        Hy2 = (U if U is not None else V).Hy
        args = (_ptr(u), _ptr(v), _ptr(U), _ptr(V), dz.data_ptr(), first.Nx, first.Ny, first.Nz, first.Hx, first.Hy, first.Hz, Hy2,
                _lib.ft_of(dtype))
        self._set_call(lib.tpg_barotropic_mode, args, _lib.check_barotropic, device, held, (U, V) if fill_halos else ())


def barotropic_mode_plan(u, v, U=None, V=None, *, fill_halos=True):
    return BarotropicModePlan(u, v, U, V, fill_halos=fill_halos)


def compute_barotropic_mode(u, v, U=None, V=None, *, fill_halos=True):
    """The barotropic mode Ū = Σ_k Δz u, V̄ = Σ_k Δz v of the 3-D velocities, summed in the fixed order k = 1..Nz (the rule of
    tpg_barotropic_mode), then (with `fill_halos`) the halo fill of the outputs.  u at (Face, Center, Center) and v at (Center, Face, Center)
    live on one TripolarGrid; their halos are not read.  `U`, `V`: the fields to write into, at (Face, Center, Nothing) and
    (Center, Face, Nothing), on the fields' grid or on its extended-halo twin; None allocates them on the fields' own grid.  Returns (U, V).
    Builds a BarotropicModePlan and runs it once; use barotropic_mode_plan in a time loop."""
    plan = BarotropicModePlan(u, v, U, V, fill_halos=fill_halos, what="compute_barotropic_mode")
    plan()
    return plan.U, plan.V


class BarotropicCorrectionPlan(OperatorPlan):
    """barotropic_correction(u, v, U, V, Ubar, Vbar) with the arguments built once: `plan()` issues, with Ubar / Vbar None, ONE
    tpg_barotropic_mode call into the plan's own planes, then ONE tpg_barotropic_correction call on torch's current stream and, with
    `fill_halos`, ONE HaloFillPlan of (u, v).  It allocates nothing when called and is a single chain of launches, so it replays inside
    torch.cuda.graph (serial grids: a seam exchange cannot be captured).  On an ImmersedBoundaryGrid with `mask_immersed` the (Face, Center)
    and (Center, Face) count planes and the value 0 go into the call.  The plan holds the tensors of the fields, the depth table and the count
    planes: rebuild it if a field's `data` is replaced."""

    def __init__(self, u, v, U, V, Ubar=None, Vbar=None, *, fill_halos=True, mask_immersed=True, what="barotropic_correction_plan"):
        for name, f in (("u", u), ("v", v), ("U", U), ("V", V)):
            if f is None:
                _require(f, name, _LOCS[name], what)
        if (Ubar is None) != (Vbar is None):
            raise TypeError(f"{what}: Ubar and Vbar are given together, or both left to the plan")
        _check({"u": u, "v": v, "U": U, "V": V, "Ubar": Ubar, "Vbar": Vbar}, what)
        self.u, self.v, self.U, self.V = u, v, U, V
        mode = ()
        if Ubar is None:                                           # the plan's own planes, beside U and V, filled by its own mode call
            Ubar, Vbar = Field(_LOCS["Ubar"], U.grid, name="Ubar"), Field(_LOCS["Vbar"], V.grid, name="Vbar")
            mode = [BarotropicModePlan(u, v, Ubar, Vbar, fill_halos=False, what=what)]
        self.Ubar, self.Vbar = Ubar, Vbar
        g = _bare(u.grid)
        dtype, device = u.data.dtype, u.data.device
        lib = _lib.barotropic_lib()
        counts = getattr(u.grid, "column_counts", None) if mask_immersed else None
        nfc, ncf = (None, None) if counts is None else (counts["fc"], counts["cf"])
        with torch.cuda.device(device):
            depth = _grid_table(g, "_column_depth_table", column_depth_table, dtype, device)
        held = [f.data for f in (u, v, U, V, Ubar, Vbar)] + [depth, nfc, ncf]
        args = (*(_ptr(t) for t in held), 0.0, u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz, U.Hy, _lib.ft_of(dtype))
        self._set_call(lib.tpg_barotropic_correction, args, _lib.check_barotropic, device, held, (u, v) if fill_halos else (), before=mode)


def barotropic_correction_plan(u, v, U, V, Ubar=None, Vbar=None, *, fill_halos=True, mask_immersed=True):
    return BarotropicCorrectionPlan(u, v, U, V, Ubar, Vbar, fill_halos=fill_halos, mask_immersed=mask_immersed)


def barotropic_correction(u, v, U, V, Ubar=None, Vbar=None, *, fill_halos=True, mask_immersed=True):
    """The split-explicit velocity correction u += (U - Ū) / H, v += (V - V̄) / H in place (the rule of tpg_barotropic_correction), which makes
    the 3-D velocities carry the sub-cycled transport (U, V), then (with `fill_halos`) the halo fill of u and v.  H is column_depth_table at the
    (Face, Center) / (Center, Face) count of the column: the full depth on a grid without a bottom.  `Ubar`, `Vbar`: the barotropic mode of
    (u, v), e.g. from compute_barotropic_mode before the sub-cycle; None computes it first.  Returns (u, v).  Builds a
    BarotropicCorrectionPlan and runs it once; use barotropic_correction_plan in a time loop."""
    BarotropicCorrectionPlan(u, v, U, V, Ubar, Vbar, fill_halos=fill_halos, mask_immersed=mask_immersed, what="barotropic_correction")()
    return u, v
