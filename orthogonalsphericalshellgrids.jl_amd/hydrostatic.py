"""The Coriolis and hydrostatic pressure-gradient tendencies of the horizontal velocities on a TripolarGrid, and the hydrostatic pressure
anomaly: what `coriolis = HydrostaticSphericalCoriolis()` and `buoyancy = BuoyancyTracer()` add to the model of the reference's drivers.
The tendency of u the AB2 step consumes becomes -U.grad(u) - f x U - d/dx p: an advection plan (momentum.py, weno_momentum.py, weno_vi.py,
weno_vs.py) leaves the first term in Gu, Gv and this module's plan continues the sum IN PLACE, left to right, as Oceananigans adds it.

Everything numeric is tpg_hydrostatic_tendencies (libtripolar_hip_hydrostatic.so): ONE launch for both fields and the pressure.  THE RULE is
written out once, in include/tripolar_hip_hydrostatic.h [recalled: Oceananigans' update_hydrostatic_pressure!, d/dx of pHY' and x_f_cross_U
/ y_f_cross_U of HydrostaticSphericalCoriolis; parity unpinned, like every operator here]: a top-down column sum of b for the pressure
anomaly PH, its two differences, and the four-point average of the transports times f in the enstrophy- or the energy-conserving form.
The rule reads u, v and b one cell beyond the interior (corners v[0, Ny+1] and u[Nx+1, 0] included) and b up to level Nz + 1: every halo is
at least 1 wide and the caller fills them first (the no-flux top halo of b is what fill_halo_regions leaves).  Only interior cells are
written.  On an ImmersedBoundaryGrid the nodes k <= n_fc[i,j] of Gu and k <= n_cf[i,j] of Gv get 0 inside the same launch; everything is
computed unmasked (Oceananigans' conditional operators beside an immersed node are out of scope).

Records: HydrostaticSphericalCoriolis(rotation_rate, scheme) with EnstrophyConserving() (the default) or EnergyConserving(), and
BuoyancyTracer().  Not built, each refused by name: SeawaterBuoyancy and equations of state (a host computes b from T and S itself and
passes it), ActiveCellEnstrophyConserving, FPlane and BetaPlane (pass a plane as `coriolis`).

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
from dataclasses import dataclass

import torch

from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _ptr, _require
from .boundary_conditions import Center, Face
from .fields import Field
from .momentum import _same
from .reductions import _bare, _grid_table, _metric, z_all_face_spacings
from .time_stepping import _on_device
from .weno_momentum import EnergyConserving, EnstrophyConserving

_LOCS = {"u": (Face, Center, Center), "v": (Center, Face, Center), "c": (Center, Center, Center)}
_BUILT = ("HydrostaticSphericalCoriolis(scheme=EnstrophyConserving()) and HydrostaticSphericalCoriolis(scheme=EnergyConserving()), or a "
          "padded (Face, Face) plane of f, are built; BuoyancyTracer() is")


@dataclass(frozen=True)
class HydrostaticSphericalCoriolis:
    """Oceananigans' `HydrostaticSphericalCoriolis(; rotation_rate, scheme)`: a plain record.  f = 2 Ω sin φ at (Face, Face)."""
    rotation_rate: float = 7.292115e-5
    scheme: object = EnstrophyConserving()


@dataclass(frozen=True)
class BuoyancyTracer:
    """Oceananigans' `BuoyancyTracer()`: the tracer b IS the buoyancy.  A plain record."""


_SCHEMES = {EnstrophyConserving: _lib.TPG_CORIOLIS_ENSTROPHY_CONSERVING, EnergyConserving: _lib.TPG_CORIOLIS_ENERGY_CONSERVING}


def _refuse_coriolis(coriolis, what):
    """the code of the scheme of a HydrostaticSphericalCoriolis record; everything else is refused by name"""
    name = type(coriolis).__name__
    if not isinstance(coriolis, HydrostaticSphericalCoriolis):
        if name in ("FPlane", "BetaPlane", "ConstantCartesianCoriolis", "NonTraditionalBetaPlane"):
            raise NotImplementedError(f"{what}: {name} is not built: pass a padded (Face, Face) plane of f as `coriolis` ({_BUILT})")
        raise NotImplementedError(f"{what}: coriolis {coriolis!r} is not built ({_BUILT})")
    if type(coriolis.scheme) not in _SCHEMES:
        raise NotImplementedError(f"{what}: the Coriolis scheme {type(coriolis.scheme).__name__} is not built "
                                  f"(ActiveCellEnstrophyConserving among them; {_BUILT})")
    return _SCHEMES[type(coriolis.scheme)]


def refuse_buoyancy(buoyancy, what="buoyancy"):
    """BuoyancyTracer() or None pass; SeawaterBuoyancy, an equation of state and everything else are refused by name"""
    if buoyancy is None or isinstance(buoyancy, BuoyancyTracer):
        return buoyancy
    raise NotImplementedError(f"{what}: {type(buoyancy).__name__} is not built: SeawaterBuoyancy and the equations of state are out of scope "
                              f"(a host computes b from T and S itself and passes it as the tracer b; {_BUILT})")


def coriolis_parameter(grid, coriolis=HydrostaticSphericalCoriolis(), dtype=None):
    """The padded (Face, Face) plane f = 2 Ω sin(φ_ff π / 180), halos included: evaluated in Float64 from the grid's own phi_ff (torch's
    sine of the product φ π/180; NOT pinned to Julia's sind, which reduces the argument in degrees -- the kernel takes f as an input plane,
    so its bits do not depend on this), rounded ONCE to `dtype` (default: the grid's), on the grid's device.  Made once per
    (grid, rotation rate, type, device) and kept with the grid, like the spacing tables.  A caller may pass any plane of that shape to the
    plans instead."""
    _refuse_coriolis(coriolis, "coriolis_parameter")
    g = _bare(grid)
    dtype = dtype or g.dtype
    rate = float(coriolis.rotation_rate)

    def build(g_, _dtype):
        phi = g_.arrays["phi_ff"].detach().to("cpu", torch.float64)
        return 2.0 * rate * torch.sin(phi * (torch.pi / 180))
    return _grid_table(g, f"_coriolis_parameter_{rate!r}", build, dtype, g.arrays["phi_ff"].device)


class HydrostaticTendenciesPlan(OperatorPlan):
    """hydrostatic_tendencies(u, v, Gu, Gv, ...) with the arguments built once: `plan()` issues ONE tpg_hydrostatic_tendencies call on
    torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of Gu and Gv.  It allocates nothing when called and is a single
    chain of launches, so it replays inside torch.cuda.graph.  `coriolis`: a HydrostaticSphericalCoriolis record, or a pair
    (plane of f at (Face, Face), scheme record), or None (no Coriolis term).  `b`: the buoyancy Field at (Center, Center, Center), halos
    filled, or None (no pressure term).  `pressure`: a Field at (Center, Center, Center) that receives the hydrostatic pressure anomaly, or
    None.  `accumulate`: add to what Gu, Gv hold (the output of an advection plan) or write.  On an ImmersedBoundaryGrid with
    `mask_immersed` the count planes and the value 0 go into the call.  The plan holds every tensor: rebuild it if a field's `data` is
    replaced."""

    def __init__(self, u, v, Gu, Gv, *, coriolis=None, b=None, pressure=None, accumulate=True, mask_immersed=True, fill_halos=False,
                 what="hydrostatic_tendencies_plan"):
        plane = None
        if isinstance(coriolis, tuple) and len(coriolis) == 2 and torch.is_tensor(coriolis[0]):
            plane, scheme = coriolis
            code = _refuse_coriolis(HydrostaticSphericalCoriolis(scheme=scheme), what)
        elif torch.is_tensor(coriolis):
            plane, code = coriolis, _lib.TPG_CORIOLIS_ENSTROPHY_CONSERVING
        elif coriolis is not None:
            code = _refuse_coriolis(coriolis, what)
        else:
            code = _lib.TPG_CORIOLIS_ENSTROPHY_CONSERVING
        if coriolis is None and b is None:
            raise ValueError(f"{what}: neither coriolis nor b: no term to compute")
        if pressure is not None and b is None:
            raise ValueError(f"{what}: pressure without b")
        names = {"u": (u, _LOCS["u"]), "v": (v, _LOCS["v"]), "Gu": (Gu, _LOCS["u"]), "Gv": (Gv, _LOCS["v"]), "b": (b, _LOCS["c"]),
                 "pressure": (pressure, _LOCS["c"])}
        first = _check_fields(names, what, "u, v, Gu, Gv, b and pressure", optional=("b", "pressure"))
        given = [(n, f) for n, (f, _) in names.items() if f is not None]
        for name, g in (("Gu", Gu), ("Gv", Gv), ("pressure", pressure)):
            for other, f in given:
                if g is None or other in ("Gu", "Gv", "pressure"):
                    continue
                if _same(g, f):
                    raise ValueError(f"{what}: {name} is {other} itself (every node reads its neighbours while they are written)")
        if _same(Gu, Gv):
            raise ValueError(f"{what}: Gu and Gv are one field")
        if any(h < 1 for h in (first.Hx, first.Hy, first.Hz)):
            raise ValueError(f"{what}: the rule reads one cell beyond the interior on every side: every halo must be at least 1 "
                             f"(halo ({first.Hx}, {first.Hy}, {first.Hz}))")
        g = _bare(first.grid)
        if g.global_size and g.Ny != g.global_size[1]:
            raise NotImplementedError(f"{what}: latitude-band grids are not handled: the rows 0 and Ny + 1 of a band are exchanged halo rows, "
                                      "and the band path of the hydrostatic tendencies is not tested yet")
        dtype, device = u.data.dtype, u.data.device
        shape = tuple(u.data.shape[-2:])
        if plane is not None and (tuple(plane.shape) != shape or plane.dtype != dtype or plane.device != device):
            raise ValueError(f"{what}: the plane of f must be a padded (Face, Face) plane of shape {shape} in the fields' element type and device")
        self.u, self.v, self.Gu, self.Gv, self.b, self.pressure = u, v, Gu, Gv, b, pressure
        function, check = _lib.hydrostatic_lib().tpg_hydrostatic_tendencies, _lib.check_hydrostatic
        counts = getattr(first.grid, "column_counts", None) if mask_immersed else None
        nfc, ncf = (None, None) if counts is None else (counts["fc"], counts["cf"])
        with _on_device(device):
            if coriolis is not None and plane is None:
                plane = coriolis_parameter(g, coriolis, dtype)
                if plane.device != device:
                    plane = plane.to(device)
            dx_fc, dy_fc, dx_cf, dy_cf = (_metric(g, name, dtype, device) for name in ("dx_fc", "dy_fc", "dx_cf", "dy_cf"))
            dz = _grid_table(g, "_z_all_face_spacings", z_all_face_spacings, dtype, device)
        plane = None if plane is None else plane.contiguous()
        held = [u.data, v.data, None if b is None else b.data, Gu.data, Gv.data, None if pressure is None else pressure.data, plane,
                dx_fc, dy_fc, dx_cf, dy_cf, dz, nfc, ncf]
        mode = _lib.TPG_TENDENCY_ADD if accumulate else _lib.TPG_TENDENCY_WRITE
        args = (*(_ptr(t) for t in held), 0.0, code, mode, u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz, _lib.ft_of(dtype))
        self._set_call(function, args, check, device, held, (Gu, Gv) if fill_halos else ())


def hydrostatic_tendencies_plan(u, v, Gu, Gv, *, coriolis=None, b=None, pressure=None, accumulate=True, mask_immersed=True, fill_halos=False):
    return HydrostaticTendenciesPlan(u, v, Gu, Gv, coriolis=coriolis, b=b, pressure=pressure, accumulate=accumulate,
                                     mask_immersed=mask_immersed, fill_halos=fill_halos)


def hydrostatic_tendencies(u, v, Gu, Gv, *, coriolis=None, b=None, pressure=None, accumulate=True, mask_immersed=True, fill_halos=False):
    """Adds (accumulate, the default) or writes the Coriolis and hydrostatic pressure-gradient tendencies to the Fields Gu at
    (Face, Center, Center) and Gv at (Center, Face, Center): the rule of tpg_hydrostatic_tendencies (include/tripolar_hip_hydrostatic.h) on
    every interior node.  u, v (and b, pressure) live on one TripolarGrid, share element type and device, and HAVE THEIR HALOS FILLED
    (corners included; b's top halo too).  Returns (Gu, Gv).  Builds a HydrostaticTendenciesPlan and runs it once; use
    hydrostatic_tendencies_plan in a time loop."""
    plan = HydrostaticTendenciesPlan(u, v, Gu, Gv, coriolis=coriolis, b=b, pressure=pressure, accumulate=accumulate,
                                     mask_immersed=mask_immersed, fill_halos=fill_halos, what="hydrostatic_tendencies")
    plan()
    return plan.Gu, plan.Gv


class HydrostaticPressurePlan(OperatorPlan):
    """update_hydrostatic_pressure(b, out) with the arguments built once: ONE tpg_hydrostatic_tendencies call with Gu = Gv = NULL."""

    def __init__(self, b, out, *, what="hydrostatic_pressure_plan"):
        first = _check_fields({"b": (b, _LOCS["c"]), "out": (out, _LOCS["c"])}, what, "b and out")
        if _same(b, out):
            raise ValueError(f"{what}: out is b itself (every column reads the levels above while they are written)")
        if any(h < 1 for h in (first.Hx, first.Hy, first.Hz)):
            raise ValueError(f"{what}: the rule reads b one level above the interior: every halo must be at least 1 "
                             f"(halo ({first.Hx}, {first.Hy}, {first.Hz}))")
        g = _bare(first.grid)
        dtype, device = b.data.dtype, b.data.device
        self.b, self.pressure = b, out
        with _on_device(device):
            dz = _grid_table(g, "_z_all_face_spacings", z_all_face_spacings, dtype, device)
        held = [None, None, b.data, None, None, out.data, None, None, None, None, None, dz, None, None]
        args = (*(_ptr(t) for t in held), 0.0, 0, _lib.TPG_TENDENCY_WRITE, b.Nx, b.Ny, b.Nz, b.Hx, b.Hy, b.Hz, _lib.ft_of(dtype))
        self._set_call(_lib.hydrostatic_lib().tpg_hydrostatic_tendencies, args, _lib.check_hydrostatic, device, held)


def update_hydrostatic_pressure(b, out=None):
    """The hydrostatic pressure anomaly PH of the buoyancy Field b (halos filled, the top halo included) as a Field at
    (Center, Center, Center): PH[Nz] = -(½ (b[Nz] + b[Nz+1])) Δz_f[Nz+1], PH[k] = PH[k+1] - (½ (b[k] + b[k+1])) Δz_f[k+1] downwards.  Only
    the interior is written.  `out`: the Field to write into; None allocates CenterField(grid)."""
    what = "update_hydrostatic_pressure"
    _require(b, "b", _LOCS["c"], what)
    out = Field(_LOCS["c"], b.grid, name="pHY") if out is None else out
    HydrostaticPressurePlan(b, out, what=what)()
    return out
