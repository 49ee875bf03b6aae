"""The vertically implicit diffusion step of a hydrostatic model on a TripolarGrid: what Oceananigans' `implicit_step!` does to u, v and
every tracer right after their AB2 update under `VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ)` -- and what every
closure with a vertically implicit diffusivity (convective adjustment, Ri-based mixing, CATKE) ends in: (1 - Δt ∂z κ ∂z) ϕ = f, one
tridiagonal system per column.

Everything numeric is tpg_vertical_implicit_diffusion (libtripolar_hip_vertical_diffusion.so): ONE launch per call, one matrix per column
and up to 16 right-hand sides, solved in place.  THE RULE is written out once, in include/tripolar_hip_vertical_diffusion.h [recalled:
Oceananigans' ivd_upper_diagonal / ivd_lower_diagonal / ivd_diagonal, κ_Δz² and solve_batched_tridiagonal_system_z!; parity unpinned, like
every operator here].  No halo cell is read or written; faces 1 and Nz + 1 carry no flux (boundary fluxes belong to the explicit tendency,
which is not built).  On an ImmersedBoundaryGrid the cells under the bottom get 0 and the system is that of the wet levels alone.

Records: VerticallyImplicitTimeDiscretization(), VerticalScalarDiffusivity(time_discretization, nu, kappa).  Not built, each refused by
name: ExplicitTimeDiscretization (the explicit diffusive tendency), HorizontalScalarDiffusivity, ConvectiveAdjustmentVerticalDiffusivity,
RiBasedVerticalDiffusivity, CATKEVerticalDiffusivity and every other closure -- a diffusivity computed by the host can be passed as a Field.

The plan form holds its tensors and its own scratch: calling it enqueues on torch's current stream and allocates nothing (usable inside
torch.cuda.graph)."""
import numbers
from collections.abc import Mapping
from dataclasses import dataclass

import torch

from . import _lib
from ._operator_plan import _check_fields, _loc_names, _ptr
from .boundary_conditions import Center, Face
from .fields import Field
from .reductions import _bare, _grid_table, z_all_face_spacings, z_center_spacings
from .time_stepping import _on_device, _SteppedPlan

_BUILT = ("VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), nu, kappa) is built, with a number, Nz + 1 face values or a "
          "Field at the fields' horizontal location and Face in z for each diffusivity: a diffusivity computed by the host can be passed as a Field")
_PATHS = {"auto": _lib.TPG_VDIFF_AUTO, "on_chip": _lib.TPG_VDIFF_ON_CHIP, "streamed": _lib.TPG_VDIFF_STREAMED}


@dataclass(frozen=True)
class VerticallyImplicitTimeDiscretization:
    """Oceananigans' `VerticallyImplicitTimeDiscretization()`: a plain record."""


@dataclass(frozen=True)
class ExplicitTimeDiscretization:
    """Oceananigans' `ExplicitTimeDiscretization()`: a plain record, refused by name wherever a closure is consumed (the explicit diffusive
    tendency is not built)."""


@dataclass(frozen=True)
class VerticalScalarDiffusivity:
    """Oceananigans' `VerticalScalarDiffusivity(time_discretization; ν, κ)`: a plain record.  `nu`: the viscosity of u and v; `kappa`: the
    diffusivity of the tracers, one value or a mapping tracer name -> value.  A value is a number, a tensor of Nz + 1 face values or a
    Field at (the field's horizontal location, Face)."""
    time_discretization: object = VerticallyImplicitTimeDiscretization()
    nu: object = 0.0
    kappa: object = 0.0


def refuse_closure(closure, what="closure"):
    """a VerticalScalarDiffusivity with the implicit discretization passes; everything else is refused by name, with what is built"""
    name = type(closure).__name__
    if isinstance(closure, VerticalScalarDiffusivity):
        disc = closure.time_discretization
        if isinstance(disc, VerticallyImplicitTimeDiscretization):
            return closure
        if isinstance(disc, ExplicitTimeDiscretization) or type(disc).__name__ == "ExplicitTimeDiscretization":
            raise NotImplementedError(f"{what}: ExplicitTimeDiscretization is not built: the explicit diffusive tendency is out of scope ({_BUILT})")
        raise NotImplementedError(f"{what}: the time discretization {disc!r} is not built ({_BUILT})")
    if isinstance(closure, (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization)):
        raise NotImplementedError(f"{what}: {name} is a time discretization, not a closure ({_BUILT})")
    if isinstance(closure, (str, numbers.Number)) or closure is None:
        raise NotImplementedError(f"{what}: closure {closure!r} is not built ({_BUILT})")
    raise NotImplementedError(f"{what}: {name} is not built ({_BUILT})")


def _count_key(loc):
    return ("f" if loc[0] is Face else "c") + ("f" if loc[1] is Face else "c")


class VerticalImplicitDiffusionPlan(_SteppedPlan):
    """vertical_implicit_diffusion(fields, kappa, dt) with the arguments built once: `plan()` issues ONE tpg_vertical_implicit_diffusion call
    per 16 fields on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of the fields.  It allocates nothing when called
    and is a single chain of launches, so it replays inside torch.cuda.graph.  `dt` is built into the arguments: `plan.with_dt(dt)` returns
    a plan over the same tensors (and the same scratch) with the new step; a captured graph is re-captured then.
    `fields`: a Field or a list of Fields at ONE horizontal location, Center in z, on one grid.  `kappa`: a number, a tensor of Nz + 1
    values at the faces 1..Nz+1 in the fields' type and device, or a Field at (the fields' horizontal location, Face).  `path`: "auto",
    "on_chip" or "streamed" (the same bits); "auto" and "streamed" need a scratch parent, which the plan allocates at construction unless
    `scratch` hands it one of the fields' shape and type (the plans of one step can share it: their calls are ordered on one stream).  On an
    ImmersedBoundaryGrid with `mask_immersed` the count plane of the fields' location and the value 0 go into the call.  The plan holds every
    tensor: rebuild it if a field's `data` is replaced."""

    _dt_index = 9

    def __init__(self, fields, kappa, dt, *, path="auto", mask_immersed=True, fill_halos=False, scratch=None,
                 what="vertical_implicit_diffusion_plan"):
        fields = [fields] if isinstance(fields, Field) else list(fields)
        if not fields:
            raise TypeError(f"{what}: no fields")
        for q, f in enumerate(fields):
            if not isinstance(f, Field):
                raise TypeError(f"{what}: field {q} must be a Field")
        loc = fields[0].loc
        if loc[2] is not Center or None in loc[:2]:
            raise TypeError(f"{what}: the fields must be Center in z at a (Center or Face, Center or Face) location (field 0 at ({_loc_names(loc)}))")
        for q, f in enumerate(fields):
            if f.loc != loc:
                raise ValueError(f"{what}: the fields of one call share one matrix, so one location: field {q} at ({_loc_names(f.loc)}) against "
                                 f"({_loc_names(loc)}); use one call per location (implicit_step_plan does)")
        names = {f"field {q}": (f, loc) for q, f in enumerate(fields)}
        kloc = (loc[0], loc[1], Face)
        if isinstance(kappa, Field):
            if kappa.loc != kloc:
                raise TypeError(f"{what}: a kappa Field must be at ({_loc_names(kloc)}), the fields' horizontal location and Face in z (it is at "
                                f"({_loc_names(kappa.loc)})): interpolating a diffusivity to the columns of u and v is the caller's job")
            names["kappa"] = (kappa, kloc)
        first = _check_fields(names, what, "the fields and kappa")
        for q, f in enumerate(fields):
            for r in range(q):
                if f is fields[r] or f.data.data_ptr() == fields[r].data.data_ptr():
                    raise ValueError(f"{what}: field {q} is field {r} itself")
        if path not in _PATHS:
            raise ValueError(f"{what}: path {path!r} is not one of 'auto', 'on_chip' and 'streamed'")
        dtype, device = first.data.dtype, first.data.device
        Nz = first.Nz
        value, form, ktensor = 0.0, _lib.TPG_KAPPA_CONSTANT, None
        if isinstance(kappa, Field):
            form, ktensor = _lib.TPG_KAPPA_FIELD, kappa.data
        elif torch.is_tensor(kappa) and kappa.dim() > 0:
            if tuple(kappa.shape) != (Nz + 1,) or kappa.dtype != dtype or kappa.device != device or not kappa.is_contiguous():
                raise ValueError(f"{what}: a kappa profile must be a contiguous tensor of Nz + 1 = {Nz + 1} face values in the fields' element type "
                                 f"and device (it is {tuple(kappa.shape)}, {kappa.dtype}, {kappa.device})")
            form, ktensor = _lib.TPG_KAPPA_PROFILE, kappa
        elif isinstance(kappa, numbers.Real) or (torch.is_tensor(kappa) and kappa.dim() == 0):
            value = float(kappa)
        else:
            raise TypeError(f"{what}: kappa must be a number, a tensor of Nz + 1 face values or a Field at ({_loc_names(kloc)}) (it is {kappa!r})")
        self.fields, self.kappa, self.dt, self.path = fields, kappa, float(dt), path
        lib = _lib.vertical_diffusion_lib()
        g = _bare(first.grid)
        counts = getattr(first.grid, "column_counts", None) if mask_immersed else None
        plane = None if counts is None else counts[_count_key(loc)]
        ft = _lib.ft_of(dtype)
        code = _PATHS[path]
        bound = lib.tpg_vertical_diffusion_on_chip_levels(min(len(fields), _lib.TPG_MAX_FIELDS), ft)
        _lib.check_vertical_diffusion(min(bound, 0))
        if path == "on_chip" and Nz > bound:
            raise ValueError(f"{what}: Nz = {Nz} is beyond the on-chip path's {bound} levels: use path='auto' or 'streamed'")
        with _on_device(device):
            dzc = _grid_table(g, "_z_center_spacings", z_center_spacings, dtype, device)
            dzf = _grid_table(g, "_z_all_face_spacings", z_all_face_spacings, dtype, device)
            # the plan's scratch, where the path taken needs one: t of the streamed path, which AUTO takes when it has one
            if path == "on_chip":
                scratch = None
            elif scratch is None:
                scratch = torch.empty_like(first.data)
            elif tuple(scratch.shape) != tuple(first.data.shape) or scratch.dtype != dtype or scratch.device != device or not scratch.is_contiguous():
                raise ValueError(f"{what}: scratch must be a contiguous tensor of the fields' parent shape {tuple(first.data.shape)}, type and device")
            self.scratch = scratch
        tail = (_ptr(ktensor), value, form, _ptr(dzc), _ptr(dzf), _ptr(plane), 0.0, float(dt), _ptr(self.scratch), code,
                first.Nx, first.Ny, first.Nz, first.Hx, first.Hy, first.Hz, ft)
        calls = []
        for f0 in range(0, len(fields), _lib.TPG_MAX_FIELDS):       # more than 16 fields go in several calls, as the AB2 step's do
            batch = fields[f0:f0 + _lib.TPG_MAX_FIELDS]
            table = _lib.ptr_table([f.data for f in batch])
            calls.append((table, (table, len(batch), *tail)))
        held = [f.data for f in fields] + [t for t in (ktensor, dzc, dzf, plane, self.scratch) if t is not None] + [c[0] for c in calls]
        before = []
        for _, args in calls[:-1]:
            p = _SteppedPlan()
            p._dt_index = self._dt_index
            p._set_call(lib.tpg_vertical_implicit_diffusion, args, _lib.check_vertical_diffusion, device, held)
            before.append(p)
        self._set_call(lib.tpg_vertical_implicit_diffusion, calls[-1][1], _lib.check_vertical_diffusion, device, held,
                       fields if fill_halos else (), before=before)


def vertical_implicit_diffusion_plan(fields, kappa, dt, *, path="auto", mask_immersed=True, fill_halos=False, scratch=None):
    return VerticalImplicitDiffusionPlan(fields, kappa, dt, path=path, mask_immersed=mask_immersed, fill_halos=fill_halos, scratch=scratch)


def vertical_implicit_diffusion(fields, kappa, dt, *, path="auto", mask_immersed=True, fill_halos=False):
    """Solves (1 - Δt ∂z κ ∂z) ϕ = f in every column of the Fields `fields`, in place: the rule of tpg_vertical_implicit_diffusion
    (include/tripolar_hip_vertical_diffusion.h).  The fields live on one TripolarGrid at one horizontal location, Center in z, and share
    element type and device; no halo is read or written.  Returns the fields.  Builds a VerticalImplicitDiffusionPlan and runs it once; use
    vertical_implicit_diffusion_plan in a time loop."""
    plan = VerticalImplicitDiffusionPlan(fields, kappa, dt, path=path, mask_immersed=mask_immersed, fill_halos=fill_halos,
                                         what="vertical_implicit_diffusion")
    plan()
    return plan.fields


class ImplicitStepPlan:
    """The implicit step of a model: the calls of implicit_step_plan in their order.  `plan()` runs them; `plan.with_dt(dt)` returns the
    same calls over the same tensors with the new step.  `plans`: the VerticalImplicitDiffusionPlans."""

    def __init__(self, plans, dt):
        self.plans, self.dt = tuple(plans), float(dt)

    def __call__(self):
        for p in self.plans:
            p()
        return self

    def with_dt(self, dt):
        return ImplicitStepPlan([p.with_dt(dt) for p in self.plans], dt)


def implicit_step_plan(u, v, tracers, closure, dt, *, path="auto", mask_immersed=True, fill_halos=False):
    """Oceananigans' `implicit_step!` of a hydrostatic model as the calls of one model step: u with ν and the (Face, Center) counts, v with
    ν and the (Center, Face) counts, the tracers with κ and the (Center, Center) counts -- tracers of equal κ in ONE call, one matrix for
    all of them.  `tracers`: a mapping name -> Field, or a list of Fields (then `closure.kappa` is one value).  u, v may be None.
    `closure`: a VerticalScalarDiffusivity with VerticallyImplicitTimeDiscretization(); every other closure is refused by name.  The
    plans share ONE scratch parent."""
    what = "implicit_step_plan"
    closure = refuse_closure(closure, what)
    kw = dict(path=path, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)
    plans = []

    def add(fields, k):                                            # the plans of the step share the first one's scratch
        plans.append(VerticalImplicitDiffusionPlan(fields, k, dt, scratch=plans[0].scratch if plans else None, **kw))
    for f in (u, v):
        if f is not None:
            add(f, closure.nu)
    named = list(tracers.items()) if isinstance(tracers, Mapping) else [(None, f) for f in (tracers or ())]
    kappa = closure.kappa
    if isinstance(kappa, Mapping):
        if not isinstance(tracers, Mapping):
            raise TypeError(f"{what}: a per-tracer kappa needs the tracers as a mapping name -> Field")
        missing = [name for name, _ in named if name not in kappa]
        if missing:
            raise KeyError(f"{what}: kappa has no entry for the tracers {missing}")
        groups = []                                               # tracers of one kappa (by identity or equal number) share a call
        for name, f in named:
            k = kappa[name]
            for group in groups:
                if group[0] is k or (isinstance(k, numbers.Real) and isinstance(group[0], numbers.Real) and float(k) == float(group[0])):
                    group[1].append(f)
                    break
            else:
                groups.append((k, [f]))
    else:
        groups = [(kappa, [f for _, f in named])] if named else []
    for k, fs in groups:
        add(fs, k)
    if not plans:
        raise TypeError(f"{what}: no fields")
    return ImplicitStepPlan(plans, dt)
