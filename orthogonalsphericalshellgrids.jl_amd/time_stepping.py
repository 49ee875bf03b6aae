"""The head of a split-explicit hydrostatic step on a TripolarGrid: the quasi-Adams-Bashforth-2 step that turns the tendencies of this step
and of the previous one into new velocities and tracers, and -- with a split-explicit free surface -- the barotropic forcing Gᵁ, Gⱽ its
sub-cycle integrates (free_surface.py), before the barotropic mode, the sub-cycle, the correction (barotropic.py) and w (continuity.py).  The
reference's drivers build HydrostaticFreeSurfaceModel(; grid, free_surface = SplitExplicitFreeSurface(grid; substeps = 30))
(examples/bickley_jet.jl:44-55), whose default time stepper is QuasiAdamsBashforth2.

Everything numeric is tpg_ab2_step_velocities / tpg_ab2_step_fields (include/tripolar_hip_timestep.h, libtripolar_hip_timestep.so): one
launch over the interior nodes, in the fields' type,
    c1 = 1.5 + χ;  c2 = 0.5 + χ;   g = c1 Gⁿ[i,j,k] - c2 G⁻[i,j,k]   (euler: g = c1 Gⁿ[i,j,k], G⁻ not read);   x[i,j,k] = x[i,j,k] + Δt g
    store_tendencies:  G⁻[i,j,k] = Gⁿ[i,j,k]
    Gᵁ[i,j] = Δzᵃᵃᶜ[1] ĝ_1;  for k = 2..Nz:  Gᵁ[i,j] = Gᵁ[i,j] + Δzᵃᵃᶜ[k] ĝ_k     ĝ_k = +0 on the peripheral nodes k <= n_fc[i,j], g elsewhere
[recalled: Oceananigans' QuasiAdamsBashforth2 ab2_step_velocities!, ab2_step_tracers!, store_tendencies! and, for a split-explicit free
surface, _compute_integrated_ab2_tendencies!; parity unpinned], followed (with `fill_halos`) by the stepped fields' own halo fill through the
plan machinery of fields.py.  Gᵁ, Gⱽ may live on another grid object than u and v -- the case that matters is the extended-halo grid of
SplitExplicitFreeSurface, whose GU, GV planes they are: they share Nx, Ny, Hx, element type and device with u, and their own north / south
halo goes into the call.  The velocities themselves are stepped unmasked: their mask is the correction's.  Latitude-band grids are accepted:
there is no stencil, and each band integrates its own columns.  The plan forms hold their tensors: calling one enqueues on torch's current
stream and allocates nothing (usable inside torch.cuda.graph)."""
import contextlib
import copy

import torch

from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _loc_names, _ptr, _require
from .boundary_conditions import Center, Face
from .fields import Field
from .grids import is_tripolar
from .reductions import _bare, _grid_table, z_center_spacings

_LOCS = {"u": (Face, Center, Center), "v": (Center, Face, Center), "GU": (Face, Center, None), "GV": (Center, Face, None)}


def _flags(euler, store_tendencies):
    return (_lib.TPG_AB2_EULER if euler else 0) | (_lib.TPG_AB2_STORE_PREVIOUS if store_tendencies else 0)


def _refuse_aliases(x, Gn, Gm, names, what):
    """a tendency that is the field itself, and this step's tendency that is the previous one's: refused by identity of the tensors"""
    same = lambda a, b: a is not None and b is not None and (a is b or a.data is b.data or a.data.data_ptr() == b.data.data_ptr())
    if same(x, Gn) or same(x, Gm):
        raise ValueError(f"{what}: a tendency of {names[0]} is the field itself")
    if same(Gn, Gm):
        raise ValueError(f"{what}: {names[1]} and {names[2]} are one field (the step reads both; store_tendencies copies one into the other)")


def _on_device(device):
    """the device context of the tables' upload; a host-only record (the argument checks) has none"""
    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()


class _SteppedPlan(OperatorPlan):
    """what both AB2 plans share: the step built into the arguments, and with_dt"""

    def with_dt(self, dt):
        """A plan over the SAME tensors with the step `dt`: nothing is allocated, only the step in the call's arguments differs.  A captured
        graph holds the old step: re-capture it with the new plan (the wizard changes Δt every 10 iterations)."""
        new = copy.copy(self)
        fn, args = self._call
        new._call = (fn, args[:self._dt_index] + (float(dt),) + args[self._dt_index + 1:])
        new._before = tuple(p.with_dt(dt) for p in self._before)
        new.dt = float(dt)
        return new


class Ab2VelocityStepPlan(_SteppedPlan):
    """ab2_step_velocities(u, v, Gu, Gv, Gu_prev, Gv_prev, dt) with the arguments built once: `plan()` issues ONE tpg_ab2_step_velocities call
    on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of (u, v).  It allocates nothing when called and is a single chain
    of launches, so it replays inside torch.cuda.graph.  `dt` and `chi` are built into the arguments: `plan.with_dt(dt)` returns a plan over
    the same tensors with the new step, and a captured graph is re-captured then (the wizard changes Δt every 10 iterations).  A group
    (u, Gu, Gu_prev, GU) or (v, Gv, Gv_prev, GV) may be None together.  On an ImmersedBoundaryGrid with `mask_immersed` the (Face, Center) and
    (Center, Face) count planes go into the call: the forcing integrates +0 on the peripheral nodes.  The plan holds the tensors of the fields,
    the spacings and the count planes: rebuild it if a field's `data` is replaced."""

    _dt_index = 11

    def __init__(self, u, v, Gu, Gv, Gu_prev, Gv_prev, dt, *, chi=0.1, GU=None, GV=None, euler=False, store_tendencies=True,
                 mask_immersed=True, fill_halos=False, what="ab2_velocity_step_plan"):
        names = {"u": (u, _LOCS["u"]), "Gu": (Gu, _LOCS["u"]), "Gu_prev": (Gu_prev, _LOCS["u"]),
                 "v": (v, _LOCS["v"]), "Gv": (Gv, _LOCS["v"]), "Gv_prev": (Gv_prev, _LOCS["v"])}
        first = _check_fields(names, what, "u, v and their tendencies", optional=tuple(names), type_group="u, v, their tendencies and Gᵁ, Gⱽ")
        if u is None and v is None:
            if GU is not None or GV is not None:
                raise TypeError(f"{what}: GU needs u and GV needs v (both of u and v are None)")
            raise TypeError(f"{what}: at least one of u at (Face, Center, Center) and v at (Center, Face, Center) is needed")
        need_prev = (not euler) or store_tendencies
        for x, Gn, Gm, G, n in ((u, Gu, Gu_prev, GU, ("u", "Gu", "Gu_prev", "GU")), (v, Gv, Gv_prev, GV, ("v", "Gv", "Gv_prev", "GV"))):
            if x is None:
                if G is not None:
                    raise TypeError(f"{what}: {n[3]} needs {n[0]} (the forcing is the integral of {n[0]}'s tendency)")
                if Gn is not None or Gm is not None:
                    raise TypeError(f"{what}: {n[0]}, {n[1]} and {n[2]} are given together (a group may be None together)")
                continue
            if Gn is None:
                raise TypeError(f"{what}: {n[0]}, {n[1]} and {n[2]} are given together (a group may be None together)")
            if Gm is None and need_prev:
                raise TypeError(f"{what}: {n[2]} is needed: store_tendencies writes it and euler=False reads it "
                                "(it may be None only with euler=True, store_tendencies=False)")
            _refuse_aliases(x, Gn, Gm, n, what)
        planes = [(n, f) for n, f in (("GU", GU), ("GV", GV)) if f is not None]
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
                raise ValueError(f"{what}: u, v, their tendencies and Gᵁ, Gⱽ must share one element type and device")
        self.u, self.v, self.GU, self.GV, self.dt, self.chi = u, v, GU, GV, float(dt), float(chi)
        g = _bare(first.grid)
        dtype, device = first.data.dtype, first.data.device
        lib = _lib.timestep_lib()
        counts = getattr(first.grid, "column_counts", None) if (mask_immersed and planes) else None
        nfc, ncf = (None, None) if counts is None else (counts["fc"] if GU is not None else None, counts["cf"] if GV is not None else None)
        dz = None
        if planes:
            with _on_device(device):
                dz = _grid_table(g, "_z_center_spacings", z_center_spacings, dtype, device)
        if not need_prev:
            Gu_prev = Gv_prev = None                                # not read, not written: not passed
        tensors = (u, v, Gu, Gv, Gu_prev, Gv_prev, GU, GV, dz, nfc, ncf)
        held = [t.data for t in tensors if t is not None]
        Hy2 = planes[0][1].Hy if planes else 0
        args = (*(_ptr(t) for t in tensors), float(dt), float(chi), _flags(euler, store_tendencies), first.Nx, first.Ny, first.Nz, first.Hx,
                first.Hy, first.Hz, Hy2, _lib.ft_of(dtype))
        self._set_call(lib.tpg_ab2_step_velocities, args, _lib.check_timestep, device, held, (u, v) if fill_halos else ())


def ab2_velocity_step_plan(u, v, Gu, Gv, Gu_prev, Gv_prev, dt, *, chi=0.1, GU=None, GV=None, euler=False, store_tendencies=True,
                           mask_immersed=True, fill_halos=False):
    return Ab2VelocityStepPlan(u, v, Gu, Gv, Gu_prev, Gv_prev, dt, chi=chi, GU=GU, GV=GV, euler=euler, store_tendencies=store_tendencies,
                               mask_immersed=mask_immersed, fill_halos=fill_halos)


def ab2_step_velocities(u, v, Gu, Gv, Gu_prev, Gv_prev, dt, *, chi=0.1, GU=None, GV=None, euler=False, store_tendencies=True,
                        mask_immersed=True, fill_halos=False):
    """The AB2 step of the velocities in place, u += Δt ((1.5 + χ) Gu - (0.5 + χ) Gu_prev) and v likewise (the rule of
    tpg_ab2_step_velocities), with `store_tendencies` then Gu_prev = Gu, and, where `GU` / `GV` are given, the barotropic forcing
    Gᵁ = Σ_k Δz ĝ, summed in the fixed order k = 1..Nz, written into them in the same launch.  u at (Face, Center, Center) and v at
    (Center, Face, Center) with their tendencies live on one TripolarGrid; no halo is read.  `GU`, `GV`: Fields at (Face, Center, Nothing) /
    (Center, Face, Nothing), on the fields' grid or on its extended-halo twin -- SplitExplicitFreeSurface's own GU, GV; only their interior
    is written, which is all tpg_free_surface_substep reads.  `euler=True`: a first step, g = (1.5 + χ) Gu, Gu_prev is not read; `chi` stays
    the caller's (Oceananigans passes χ = -0.5 then, which makes the factor one).  On an ImmersedBoundaryGrid with `mask_immersed` the
    forcing integrates +0 on the peripheral nodes; u and v themselves are stepped unmasked (the correction masks them).  Returns (u, v).
    Builds an Ab2VelocityStepPlan and runs it once; use ab2_velocity_step_plan in a time loop."""
    Ab2VelocityStepPlan(u, v, Gu, Gv, Gu_prev, Gv_prev, dt, chi=chi, GU=GU, GV=GV, euler=euler, store_tendencies=store_tendencies,
                        mask_immersed=mask_immersed, fill_halos=fill_halos, what="ab2_step_velocities")()
    return u, v


class Ab2StepPlan(_SteppedPlan):
    """ab2_step_fields(fields, Gn, Gm, dt) with the arguments built once: `plan()` issues ONE tpg_ab2_step_fields call per 16 fields on
    torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of the fields.  It allocates nothing when called and is a single
    chain of launches, so it replays inside torch.cuda.graph.  `dt` and `chi` are built into the arguments: `plan.with_dt(dt)` returns a
    plan over the same tensors with the new step, and a captured graph is re-captured then (the wizard changes Δt every 10 iterations).
    The plan holds the tensors of the fields: rebuild it if a field's `data` is replaced."""

    _dt_index = 4

    def __init__(self, fields, Gn, Gm, dt, *, chi=0.1, euler=False, store_tendencies=True, fill_halos=False, what="ab2_step_plan"):
        fields, Gn = list(fields), list(Gn)
        need_prev = (not euler) or store_tendencies
        if Gm is None:
            if need_prev:
                raise TypeError(f"{what}: Gm is needed: store_tendencies writes it and euler=False reads it "
                                "(it may be None only with euler=True, store_tendencies=False)")
            Gm = [None] * len(fields)
        Gm = list(Gm)
        if not fields:
            raise TypeError(f"{what}: no fields")
        if not (len(fields) == len(Gn) == len(Gm)):
            raise TypeError(f"{what}: fields, Gn and Gm are lists of one length ({len(fields)}, {len(Gn)}, {len(Gm)})")
        for q, f in enumerate(fields):
            if not isinstance(f, Field):
                raise TypeError(f"{what}: field {q} must be a Field")
        names = {}
        for q, (f, n, m) in enumerate(zip(fields, Gn, Gm)):
            names.update({f"field {q}": (f, f.loc), f"Gn of field {q}": (n, f.loc), f"Gm of field {q}": (m, f.loc)})
        optional = () if need_prev else tuple(k for k in names if k.startswith("Gm"))
        first = _check_fields(names, what, "the fields and their tendencies", optional=optional)
        for q, (f, n, m) in enumerate(zip(fields, Gn, Gm)):
            if tuple(f.data.shape) != tuple(first.data.shape):
                raise ValueError(f"{what}: the fields must share one location's geometry (field {q} at ({_loc_names(f.loc)}) has the parent "
                                 f"{tuple(f.data.shape)} against {tuple(first.data.shape)})")
            _refuse_aliases(f, n, m, (f"field {q}", f"Gn of field {q}", f"Gm of field {q}"), what)
        self.fields, self.dt, self.chi = fields, float(dt), float(chi)
        dtype, device = first.data.dtype, first.data.device
        lib = _lib.timestep_lib()
        if not need_prev:
            Gm = [None] * len(fields)
        tail = (float(chi), _flags(euler, store_tendencies), first.Nx, first.Ny, first.Nz, first.Hx, first.Hy, first.Hz, _lib.ft_of(dtype))
        calls = []
        for f0 in range(0, len(fields), _lib.TPG_MAX_FIELDS):       # more than 16 fields go in several calls, as the fill's do
            sl = slice(f0, f0 + _lib.TPG_MAX_FIELDS)
            tables = [_lib.ptr_table([t.data for t in fields[sl]]), _lib.ptr_table([t.data for t in Gn[sl]]),
                      _lib.ptr_table([t.data for t in Gm[sl]]) if need_prev else None]
            calls.append((tables, (*tables, len(fields[sl]), float(dt), *tail)))
        held = [t.data for t in (*fields, *Gn, *Gm) if t is not None] + [c[0] for c in calls]
        before = []
        for _, args in calls[:-1]:
            p = _SteppedPlan()
            p._dt_index = self._dt_index
            p._set_call(lib.tpg_ab2_step_fields, args, _lib.check_timestep, device, held)
            before.append(p)
        self._set_call(lib.tpg_ab2_step_fields, calls[-1][1], _lib.check_timestep, device, held, fields if fill_halos else (), before=before)


def ab2_step_plan(fields, Gn, Gm, dt, *, chi=0.1, euler=False, store_tendencies=True, fill_halos=False):
    return Ab2StepPlan(fields, Gn, Gm, dt, chi=chi, euler=euler, store_tendencies=store_tendencies, fill_halos=fill_halos)


def ab2_step_fields(fields, Gn, Gm, dt, *, chi=0.1, euler=False, store_tendencies=True, fill_halos=False):
    """The AB2 step of any fields of one grid, one location's geometry and one type -- the tracers -- in place:
    c += Δt ((1.5 + χ) Gn - (0.5 + χ) Gm), with `store_tendencies` then Gm = Gn (the rule of tpg_ab2_step_fields); no integral, no mask.
    `fields`, `Gn`, `Gm`: lists of one length, each tendency a Field at its field's location; `Gm` may be None with euler=True and
    store_tendencies=False.  More than 16 fields go in several calls.  Returns the fields.  Builds an Ab2StepPlan and runs it once; use
    ab2_step_plan in a time loop."""
    plan = Ab2StepPlan(fields, Gn, Gm, dt, chi=chi, euler=euler, store_tendencies=store_tendencies, fill_halos=fill_halos, what="ab2_step_fields")
    plan()
    return plan.fields
