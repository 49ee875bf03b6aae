"""The vertical mixing closures of a hydrostatic model on a TripolarGrid that react to the column: convective adjustment and
Richardson-number-based mixing.  Both compute a diffusivity and a viscosity at the cell interfaces from b (and u, v), and end in the column
solve of vertical_diffusion.py: this module computes them ON THE DEVICE at the three locations the implicit step's FIELD form wants -- κ
and ν at (Center, Center, Face), ν interpolated to the columns of u, (Face, Center, Face), and of v, (Center, Face, Face) -- and chains the
three implicit calls behind them (mixed_implicit_step_plan).

Everything numeric is tpg_convective_adjustment_diffusivities / tpg_ri_based_diffusivities (libtripolar_hip_mixing.so): ONE launch per call.
THE RULE is written out once, in csrc/staged/tripolar_hip_mixing.h [recalled: Oceananigans' ConvectiveAdjustmentVerticalDiffusivity and
RiBasedVerticalDiffusivity with PiecewiseLinearRiDependentTapering; parity unpinned, like every operator here].  b, u and v are read one cell
beyond the interior: the caller HAS FILLED their horizontal halos.

The library is STAGED beside the table of _lib.LIBRARIES, whose size is pinned: this module binds it itself with _lib._load, holds its
signature table and MIXING_LIB_PATH (which a caller may assign before the first load), and fails as loudly when the file is missing.

Records: ConvectiveAdjustmentVerticalDiffusivity, RiBasedVerticalDiffusivity (its defaults are Oceananigans' as recalled: the hyperbolic
tangent taper and Cen = 0.1, which this build refuses -- pass PiecewiseLinearRiDependentTapering() and Cen=0), and the three tapering
records.  The refusals of vertical_diffusion.refuse_closure and of diffusion.py still name these closures as not built: their messages are
pinned and out of date.

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
import ctypes as C
import math
import numbers
import os
from collections.abc import Mapping
from dataclasses import dataclass

import torch

from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _loc_names, _ptr
from .boundary_conditions import Center, Face
from .fields import Field
from .reductions import _bare, _grid_table, z_all_face_spacings
from .time_stepping import _on_device
from .vertical_diffusion import VerticalImplicitDiffusionPlan, VerticallyImplicitTimeDiscretization

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
# every symbol csrc/staged/tripolar_hip_mixing.h declares, (restype, argtypes)
MIXING_SIGNATURES = {
    "tpg_mixing_last_error": (C.c_char_p, []),
    "tpg_convective_adjustment_diffusivities": (_i, [_vp] * 5 + [_d] * 4 + [_vp] * 4 + [_d] + [_i] * 6 + [_i, _vp]),
    "tpg_ri_based_diffusivities": (_i, [_vp] * 9 + [_d] * 6 + [_vp] * 4 + [_d] + [_i] * 6 + [_i, _vp]),
}
MIXING_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtripolar_hip_mixing.so")
_mixing = None

BUILT = ("ConvectiveAdjustmentVerticalDiffusivity(VerticallyImplicitTimeDiscretization(), convective_kappa_z, convective_nu_z, "
         "background_kappa_z, background_nu_z) with numbers, and RiBasedVerticalDiffusivity(VerticallyImplicitTimeDiscretization(), "
         "Ri_dependent_tapering=PiecewiseLinearRiDependentTapering(), Cen=0, horizontal_Ri_filter=None) with numbers are built")
OUTPUTS = ("kappa_c", "nu_c", "kappa_u", "kappa_v")
_OUTPUT_LOCS = {"kappa_c": (Center, Center, Face), "nu_c": (Center, Center, Face), "kappa_u": (Face, Center, Face), "kappa_v": (Center, Face, Face)}


def mixing_lib():
    """Load the library at MIXING_LIB_PATH (once); ImportError if it has not been built."""
    global _mixing
    if _mixing is None:
        _mixing = _lib._load(MIXING_LIB_PATH, MIXING_SIGNATURES)
    return _mixing


def check_mixing(status):
    if status != 0:
        raise _lib.TripolarHipError(status, mixing_lib().tpg_mixing_last_error().decode("utf-8", "replace"))


@dataclass(frozen=True)
class PiecewiseLinearRiDependentTapering:
    """Oceananigans' `PiecewiseLinearRiDependentTapering()`: tau = 1 - min(1, max(0, (Ri - Ri0) / Ri_delta)).  The one that is built."""


@dataclass(frozen=True)
class HyperbolicTangentRiDependentTapering:
    """Oceananigans' `HyperbolicTangentRiDependentTapering()`: a plain record, refused by name where it is consumed."""


@dataclass(frozen=True)
class ExponentialRiDependentTapering:
    """Oceananigans' `ExponentialRiDependentTapering()`: a plain record, refused by name where it is consumed."""


@dataclass(frozen=True)
class ConvectiveAdjustmentVerticalDiffusivity:
    """Oceananigans' `ConvectiveAdjustmentVerticalDiffusivity(time_discretization; convective_κz, convective_νz, background_κz,
    background_νz)`: a plain record of four numbers.  Where ∂z b < 0 (or is NaN) at an interface the convective values hold, elsewhere the
    background values."""
    time_discretization: object = VerticallyImplicitTimeDiscretization()
    convective_kappa_z: object = 0.0
    convective_nu_z: object = 0.0
    background_kappa_z: object = 0.0
    background_nu_z: object = 0.0


@dataclass(frozen=True)
class RiBasedVerticalDiffusivity:
    """Oceananigans' `RiBasedVerticalDiffusivity(time_discretization; Ri_dependent_tapering, horizontal_Ri_filter, ν₀, κ₀, κᶜᵃ, Cᵉⁿ, Cᵃᵛ, Ri₀,
    Riᵟ)`: a plain record; the defaults are Oceananigans' [recalled].  Built: the piecewise-linear taper without entrainment and without
    the horizontal filter; the record's defaults (hyperbolic tangent, Cen = 0.1) are therefore refused at plan time."""
    time_discretization: object = VerticallyImplicitTimeDiscretization()
    Ri_dependent_tapering: object = HyperbolicTangentRiDependentTapering()
    horizontal_Ri_filter: object = None
    nu0: object = 0.7
    kappa0: object = 0.5
    kappa_ca: object = 1.7
    Cen: object = 0.1
    Cav: object = 0.6
    Ri0: object = 0.1
    Ri_delta: object = 0.4


def _number(x, name, what):
    if not isinstance(x, numbers.Real) or isinstance(x, bool):
        raise NotImplementedError(f"{what}: {name} = {x!r} is not built: every parameter of the closure is one number ({BUILT})")
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"{what}: {name} = {x!r} is not finite")
    return x


def mixing_parameters(closure, what="vertical_mixing_plan"):
    """("ca" | "ri", the numbers of the C call in its order) of a closure this build serves; everything else is refused by name, with what
    is built"""
    name = type(closure).__name__
    if not isinstance(closure, (ConvectiveAdjustmentVerticalDiffusivity, RiBasedVerticalDiffusivity)):
        if name in ("CATKEVerticalDiffusivity", "TKEDissipationVerticalDiffusivity"):
            raise NotImplementedError(f"{what}: {name} is not built: no prognostic turbulent kinetic energy here ({BUILT})")
        raise NotImplementedError(f"{what}: {name} is not built as a vertical mixing closure ({BUILT})")
    disc = closure.time_discretization
    if not isinstance(disc, VerticallyImplicitTimeDiscretization):
        raise NotImplementedError(f"{what}: {name} with the time discretization {disc!r} is not built: the diffusivities go into the "
                                  f"vertically implicit step ({BUILT})")
    if isinstance(closure, ConvectiveAdjustmentVerticalDiffusivity):
        return "ca", tuple(_number(getattr(closure, k), k, what) for k in
                           ("background_kappa_z", "convective_kappa_z", "background_nu_z", "convective_nu_z"))
    taper = closure.Ri_dependent_tapering
    if not isinstance(taper, PiecewiseLinearRiDependentTapering):
        raise NotImplementedError(f"{what}: {type(taper).__name__} is not built: PiecewiseLinearRiDependentTapering() is the taper of "
                                  f"tpg_ri_based_diffusivities ({BUILT})")
    if closure.horizontal_Ri_filter is not None:
        raise NotImplementedError(f"{what}: the horizontal Ri filter {closure.horizontal_Ri_filter!r} is not built: pass "
                                  f"horizontal_Ri_filter=None ({BUILT})")
    if _number(closure.Cen, "Cen", what) != 0.0:
        raise NotImplementedError(f"{what}: the entrainment term (Cen = {closure.Cen!r}) is not built: pass Cen=0 ({BUILT})")
    q = tuple(_number(getattr(closure, k), k, what) for k in ("nu0", "kappa0", "kappa_ca", "Ri0", "Ri_delta", "Cav"))
    if q[4] <= 0:
        raise ValueError(f"{what}: Ri_delta = {q[4]!r} must be positive")
    if 1.0 + q[5] == 0.0:
        raise ValueError(f"{what}: Cav = {q[5]!r}: the time average divides by 1 + Cav")
    return "ri", q


class VerticalMixingPlan(OperatorPlan):
    """vertical_mixing_diffusivities(closure, b, u, v, ...) with the arguments built once: `plan()` issues ONE call of the closure's entry
    point on torch's current stream, then -- with `fill_halos` -- ONE HaloFillPlan of kappa_c and nu_c, then, with a time average
    (RiBasedVerticalDiffusivity with Cav != 0), copies both into the plan's twins.  It allocates nothing when called and is a single chain
    of launches, so it replays inside torch.cuda.graph.
    `b`: the buoyancy at (Center, Center, Center); `u`, `v`: the velocities, for RiBasedVerticalDiffusivity only; their horizontal halos
    HAVE BEEN FILLED.  Each output -- kappa_c, nu_c at (Center, Center, Face), kappa_u at (Face, Center, Face), kappa_v at (Center, Face,
    Face) -- is a Field there (written), True (a Field the plan allocates at construction) or None (absent); `plan.outputs` maps the names
    to the Fields.  The time average reads the previous κ and ν of the cell centres one column west and one row south: the plan OWNS the
    ping-pong twins of kappa_c and nu_c (both are then required, and `fill_halos`), zero at construction -- the first call averages with
    zero, as a model that starts from zero diffusivities does.  On an ImmersedBoundaryGrid with `mask_immersed` the three count planes and
    the value 0 go into the call.  The plan holds every tensor: rebuild it if a field's `data` is replaced."""

    def __init__(self, closure, b, u=None, v=None, *, kappa_c=True, nu_c=True, kappa_u=True, kappa_v=True, mask_immersed=True,
                 fill_halos=True, what="vertical_mixing_plan"):
        kind, q = mixing_parameters(closure, what)
        names = {"b": (b, (Center, Center, Center))}
        if kind == "ri":
            if u is None or v is None:
                raise TypeError(f"{what}: RiBasedVerticalDiffusivity needs u and v (the shear)")
            names.update({"u": (u, (Face, Center, Center)), "v": (v, (Center, Face, Center))})
        elif u is not None or v is not None:
            raise TypeError(f"{what}: ConvectiveAdjustmentVerticalDiffusivity reads b alone: u and v must be None")
        given = {"kappa_c": kappa_c, "nu_c": nu_c, "kappa_u": kappa_u, "kappa_v": kappa_v}
        for name, f in given.items():
            if f is not None and f is not True and f is not False:
                names[name] = (f, _OUTPUT_LOCS[name])
        first = _check_fields(names, what, "b, u, v and the diffusivities")
        if all(f is None or f is False for f in given.values()):
            raise TypeError(f"{what}: no output: kappa_c, nu_c, kappa_u and kappa_v are all absent")
        if first.Hx < 1 or first.Hy < 1:
            raise ValueError(f"{what}: the rule reads one cell beyond the interior west, east, south and north: Hx and Hy must be at least 1 "
                             f"(halo ({first.Hx}, {first.Hy}, {first.Hz}))")
        g = _bare(first.grid)
        if g.global_size and g.Ny != g.global_size[1]:
            raise NotImplementedError(f"{what}: latitude-band grids are not handled: the rows 0 and Ny + 1 of a band are exchanged halo rows, and "
                                      "the band path of the plan is not tested yet (the C call serves a band whose seam halos are filled)")
        averaged = kind == "ri" and q[5] != 0.0
        if averaged and (given["kappa_c"] in (None, False) or given["nu_c"] in (None, False) or not fill_halos):
            raise TypeError(f"{what}: the time average (Cav = {q[5]!r}) reads the previous kappa_c and nu_c with their filled halos: both "
                            "outputs and fill_halos are required (Cav=0 computes the instantaneous values)")
        dtype, device = first.data.dtype, first.data.device
        outputs = {}
        for name, f in given.items():
            if f is True:
                f = Field(_OUTPUT_LOCS[name], first.grid, name=name)
            outputs[name] = f if isinstance(f, Field) else None
        fields = [f for f in outputs.values() if f is not None]
        for n, f in enumerate(fields):
            for r in range(n):
                if f is fields[r] or f.data.data_ptr() == fields[r].data.data_ptr():
                    raise ValueError(f"{what}: two outputs are one field")
        self.closure, self.b, self.u, self.v, self.outputs, self.averaged = closure, b, u, v, outputs, averaged
        lib = mixing_lib()
        counts = getattr(first.grid, "column_counts", None) if mask_immersed else None
        planes = [None if counts is None else counts[k] for k in ("cc", "fc", "cf")]
        self.twins = None
        with _on_device(device):
            dzf = _grid_table(g, "_z_all_face_spacings", z_all_face_spacings, dtype, device)
            if averaged:
                self.twins = (torch.zeros_like(outputs["kappa_c"].data), torch.zeros_like(outputs["nu_c"].data))
        tail = (_ptr(dzf), *(_ptr(t) for t in planes), 0.0, b.Nx, b.Ny, b.Nz, b.Hx, b.Hy, b.Hz, _lib.ft_of(dtype))
        outs = tuple(_ptr(outputs[k]) for k in OUTPUTS)
        if kind == "ca":
            fn, args = lib.tpg_convective_adjustment_diffusivities, (_ptr(b), *outs, *q, *tail)
        else:
            prev = (None, None) if self.twins is None else tuple(t.data_ptr() for t in self.twins)
            fn, args = lib.tpg_ri_based_diffusivities, (_ptr(b), _ptr(u), _ptr(v), *prev, *outs, *q, *tail)
        held = [f.data for f in (b, u, v, *fields) if f is not None] + [t for t in (dzf, *planes, *(self.twins or ())) if t is not None]
        self._set_call(fn, args, check_mixing, device, held, [outputs["kappa_c"], outputs["nu_c"]] if fill_halos else ())

    def __call__(self):
        super().__call__()
        if self.twins is not None:                                 # this call's values, with their filled halos, are the next call's previous ones
            self.twins[0].copy_(self.outputs["kappa_c"].data)
            self.twins[1].copy_(self.outputs["nu_c"].data)
        return self


def vertical_mixing_plan(closure, b, u=None, v=None, *, kappa_c=True, nu_c=True, kappa_u=True, kappa_v=True, mask_immersed=True, fill_halos=True):
    return VerticalMixingPlan(closure, b, u, v, kappa_c=kappa_c, nu_c=nu_c, kappa_u=kappa_u, kappa_v=kappa_v, mask_immersed=mask_immersed,
                              fill_halos=fill_halos)


def vertical_mixing_diffusivities(closure, b, u=None, v=None, *, kappa_c=True, nu_c=True, kappa_u=True, kappa_v=True, mask_immersed=True,
                                  fill_halos=True):
    """The diffusivities of `closure` from b (and u, v), as a dict name -> Field of those of kappa_c, nu_c, kappa_u, kappa_v that are
    wanted: the rule of csrc/staged/tripolar_hip_mixing.h on every interior column.  Builds a VerticalMixingPlan and runs it once (a time
    average starts from zero); use vertical_mixing_plan in a time loop."""
    plan = VerticalMixingPlan(closure, b, u, v, kappa_c=kappa_c, nu_c=nu_c, kappa_u=kappa_u, kappa_v=kappa_v, mask_immersed=mask_immersed,
                              fill_halos=fill_halos, what="vertical_mixing_diffusivities")
    plan()
    return {k: f for k, f in plan.outputs.items() if f is not None}


class MixedImplicitStepPlan:
    """The implicit step of a model under a mixing closure: `mixing`, the VerticalMixingPlan, then `plans`, the
    VerticalImplicitDiffusionPlans in their FIELD form.  `plan()` runs them in that order; `plan.with_dt(dt)` returns the same calls over
    the same tensors with the new step."""

    def __init__(self, mixing, plans, dt):
        self.mixing, self.plans, self.dt = mixing, tuple(plans), float(dt)

    def __call__(self):
        self.mixing()
        for p in self.plans:
            p()
        return self

    def with_dt(self, dt):
        return MixedImplicitStepPlan(self.mixing, [p.with_dt(dt) for p in self.plans], dt)


def mixed_implicit_step_plan(closure, u, v, tracers, b, dt, *, path="auto", mask_immersed=True, fill_halos=False):
    """Oceananigans' `compute_diffusivities!` and `implicit_step!` of a hydrostatic model under ConvectiveAdjustmentVerticalDiffusivity or
    RiBasedVerticalDiffusivity as the calls of one model step: ONE diffusivity call from b (and u, v), then u with ν at its own columns,
    v with ν at its own, and the tracers with κ -- all of them in ONE call, one matrix.  `tracers`: a mapping name -> Field or a list of
    Fields (b is usually one of them); u and v may both be None for convective adjustment.  The horizontal halos of b, u and v HAVE BEEN
    FILLED.  `fill_halos`: of the stepped fields, afterwards.  The plans share ONE scratch parent."""
    what = "mixed_implicit_step_plan"
    kind, _ = mixing_parameters(closure, what)
    fields = list(tracers.values()) if isinstance(tracers, Mapping) else list(tracers or ())
    if u is None and v is None and not fields:
        raise TypeError(f"{what}: no fields")
    if kind == "ri" and (u is None or v is None):
        raise TypeError(f"{what}: RiBasedVerticalDiffusivity needs u and v (the shear)")
    mixing = VerticalMixingPlan(closure, b, u if kind == "ri" else None, v if kind == "ri" else None, kappa_c=True if fields or kind == "ri" else None,
                                nu_c=True if kind == "ri" else None, kappa_u=True if u is not None else None,
                                kappa_v=True if v is not None else None, mask_immersed=mask_immersed, what=what)
    kw = dict(path=path, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)
    plans = []
    for f, k in ((u, "kappa_u"), (v, "kappa_v"), (fields, "kappa_c")):
        if f is not None and f != []:
            plans.append(VerticalImplicitDiffusionPlan(f, mixing.outputs[k], dt, scratch=plans[0].scratch if plans else None, **kw))
    return MixedImplicitStepPlan(mixing, plans, dt)
