"""Device reductions on a TripolarGrid: what the reference's model drivers run between steps (examples/bickley_jet.jl:75,84,87;
examples/distributed_bickley_jet.jl:77,92) -- maximum(u), maximum(v) in the progress callback, TimeStepWizard's cell_advection_timescale --
and the six metric reductions that the `show` of a grid prints (the reference's README.md:54-59).

Everything numeric is tpg_field_extrema / tpg_cell_advection_timescale (include/tripolar_hip.h): one pass over the interior, one partial per
block into a workspace, a second tiny launch; min and max only, so the results are exact and compare bit for bit with a host reference.
The plan forms hold the output tensor and the workspace: calling a plan enqueues on torch's current stream and allocates nothing (usable
inside torch.cuda.graph); `result()` synchronises and returns Python floats.

Latitude-band (Distributed) grids: every reduction here covers the band's own rows.  The MIN / MAX across the ranks of the chain is the
host's (one all-reduce of a few doubles) and is not part of this module.
"""
import ctypes as C
import math

import torch

from . import _lib
from .boundary_conditions import Center, Face
from .fields import Field, _loc_code, _run
from .grids import _z_coordinate, is_tripolar


def _bare(grid):
    return getattr(grid, "underlying_grid", grid)


def _z_spec_values(grid):
    """grid.z_spec as a Python list: the two ends of a regular interval, or the explicit faces"""
    z = _bare(grid).z_spec
    return z.flatten().tolist() if torch.is_tensor(z) else list(z)


def _grid_table(grid, key, build, dtype, device):
    """the device copy of the host table build(grid, dtype), made once per (grid, type, device) and kept with the grid under `key`"""
    g = _bare(grid)
    cache = g.__dict__.setdefault(key, {})
    if (dtype, str(device)) not in cache:
        cache[(dtype, str(device))] = build(g, dtype).to(dtype).to(device)
    return cache[(dtype, str(device))]


def _workspace(lib, n, geom, device):
    nbytes = int(lib.tpg_reduce_workspace_bytes(n, geom[0], geom[1], geom[2]))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def _extrema_call(lib, tensors, geom, planes, zlocs, held):
    """(call, out) of tpg_field_extrema for `tensors` of one geometry; planes: None, or per tensor a count plane or None"""
    n = len(tensors)
    device = tensors[0].device
    with torch.cuda.device(device):
        out = torch.empty(3 * n, dtype=torch.float64, device=device)
        ws = _workspace(lib, n, geom, device)
    held.extend([out, ws, *tensors])
    counts = zl = None
    if planes is not None and any(p is not None for p in planes):
        held.extend(p for p in planes if p is not None)
        counts = (C.c_void_p * n)(*[None if p is None else p.data_ptr() for p in planes])
        zl = (C.c_int8 * n)(*zlocs)
    args = (_lib.ptr_table(tensors), n, counts, zl, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, *geom, _lib.ft_of(tensors[0].dtype))
    return (lib.tpg_field_extrema, args), out


def _triples(out):
    v = out.tolist()                                               # a device-to-host copy on the current stream: waits for the call
    return [tuple(v[3 * f:3 * f + 3]) for f in range(len(v) // 3)]


class ExtremaPlan:
    """field_extrema with everything that does not change from call to call built once: the grouping by geometry (as fill_halo_regions
    groups), the pointer tables, one output tensor and one workspace per group.  `plan()` issues one tpg_field_extrema call per group on
    torch's current stream and allocates nothing; `plan.result()` synchronises and returns one (min, max, max|c|) of Python floats per field,
    in the order the fields were given.  The plan holds the fields' tensors: rebuild it if a field's `data` is replaced."""

    def __init__(self, fields, not_immersed=True):
        if isinstance(fields, Field):
            fields = [fields]
        self.fields = list(fields)
        if not self.fields:
            raise ValueError("field_extrema: no fields")
        self._held, self._steps, self._outs = [], [], []
        lib = _lib.lib()
        groups = {}
        for index, f in enumerate(self.fields):
            if not isinstance(f, Field):
                raise TypeError(f"field_extrema: {f!r} is not a Field")
            groups.setdefault((f.data.dtype, f.data.device, f.Nx, f.Ny, f.Nz, f.Hx, f.Hy, f.Hz, id(f.grid)), []).append((index, f))
        for members in groups.values():
            fs = [f for _, f in members]
            f0 = fs[0]
            counts = getattr(f0.grid, "column_counts", None) if not_immersed else None
            planes = zlocs = None
            if counts is not None:
                for f in fs:
                    if f.loc[2] is None or f.z_window is not None or None in f.loc[:2]:
                        raise NotImplementedError("field_extrema: reduced and z-windowed fields are not handled with the NotImmersed condition "
                                                  "(as mask_immersed_field refuses them); pass not_immersed=False")
                planes = [counts[("f" if f.loc[0] is Face else "c") + ("f" if f.loc[1] is Face else "c")] for f in fs]
                zlocs = [_loc_code(f.loc[2]) for f in fs]
            call, out = _extrema_call(lib, [f.data for f in fs], (f0.Nx, f0.Ny, f0.Nz, f0.Hx, f0.Hy, f0.Hz), planes, zlocs, self._held)
            self._steps.append((f0.data.device, [call]))
            self._outs.append(([i for i, _ in members], out))

    def __call__(self):
        for device, calls in self._steps:
            _run(device, calls)
        return self

    def result(self):
        res = [None] * len(self.fields)
        for indices, out in self._outs:
            for i, t in zip(indices, _triples(out)):
                res[i] = t
        return res


def extrema_plan(fields, not_immersed=True):
    return ExtremaPlan(fields, not_immersed)


def field_extrema(fields, not_immersed=True):
    """One (min, max, max|c|) of Python floats per field, over the interior i = 1..Nx, j = 1..Ny, k = 1..Nz' (no halo cell counts; a NaN in a
    counted cell makes the field's three values NaN, as Julia's minimum / maximum do).  On an ImmersedBoundaryGrid with `not_immersed` the
    nodes that mask_immersed_field writes are left out (Oceananigans' NotImmersed condition [recalled; parity unpinned on the nodes that are
    peripheral through the domain's own walls only]); an empty set gives (+inf, -inf, -inf).  One tpg_field_extrema call per geometry
    group.  On a latitude-band grid: the band's own rows (the cross-rank MIN / MAX is the host's)."""
    return ExtremaPlan(fields, not_immersed)().result()


def minimum(field, not_immersed=True):
    """minimum(field)"""
    return field_extrema([field], not_immersed)[0][0]


def maximum(field, abs=False, not_immersed=True):
    """maximum(field), or maximum(abs, field) with abs=True"""
    return field_extrema([field], not_immersed)[0][2 if abs else 1]


# -------------------------------------------------------------------------------------------------
# cell_advection_timescale and the time-step wizard
# -------------------------------------------------------------------------------------------------
def z_face_spacings(grid, dtype=None):
    """Δzᵃᵃᶠ[k] for k = 1..Nz: the centre-to-centre spacing at face k (the centre below face 1 is a halo centre), computed in float64 from
    grid.z_spec and rounded ONCE to `dtype` (default: the grid's), as boundary_z_spacings computes its two faces -- whose first value is this
    function's k = 1.  A regular interval (z0, z1) gives (z1 - z0) / Nz at every face; explicit faces give the float64 differences of the
    adjacent float64 centres, the halo centre from the faces extrapolated as the grid's z coordinate is.  A float64 host tensor of values
    that are exact in `dtype`."""
    g = _bare(grid)
    Nz = g.Nz
    zz = _z_spec_values(g)
    if len(zz) == 2:
        d = torch.full((Nz,), (float(zz[1]) - float(zz[0])) / Nz, dtype=torch.float64)
    else:
        _, _, c = _z_coordinate(zz, Nz, 1, torch.float64, "cpu")         # centres k = 0 .. Nz+1
        d = c[1:Nz + 1] - c[0:Nz]
    return d.to(dtype or g.dtype).to(torch.float64)


def z_all_face_spacings(grid, dtype=None):
    """Δzᵃᵃᶠ[k] for k = 1..Nz+1: z_face_spacings with the top face, whose centre above is a halo centre as the centre below face 1 is (the
    vertical terms of the momentum tendency difference u and v across every face of the interior).  The first Nz values are
    z_face_spacings' bit for bit; the same float64 arithmetic, rounded ONCE to `dtype`.  A float64 host tensor of values exact in `dtype`."""
    g = _bare(grid)
    Nz = g.Nz
    zz = _z_spec_values(g)
    if len(zz) == 2:
        d = torch.full((Nz + 1,), (float(zz[1]) - float(zz[0])) / Nz, dtype=torch.float64)
    else:
        _, _, c = _z_coordinate(zz, Nz, 1, torch.float64, "cpu")         # centres k = 0 .. Nz+1
        d = c[1:Nz + 2] - c[0:Nz + 1]
    return d.to(dtype or g.dtype).to(torch.float64)


def z_center_spacings(grid, dtype=None):
    """Δzᵃᵃᶜ[k] for k = 1..Nz: the face-to-face spacing at centre k, computed in float64 from grid.z_spec and rounded ONCE to `dtype` (default:
    the grid's), as z_face_spacings is.  A regular interval (z0, z1) gives (z1 - z0) / Nz at every level; explicit faces give the float64
    differences of adjacent faces.  A float64 host tensor of values that are exact in `dtype`."""
    g = _bare(grid)
    Nz = g.Nz
    zz = _z_spec_values(g)
    if len(zz) == 2:
        d = torch.full((Nz,), (float(zz[1]) - float(zz[0])) / Nz, dtype=torch.float64)
    else:
        f = torch.tensor([float(z) for z in zz], dtype=torch.float64)
        d = f[1:Nz + 1] - f[0:Nz]
    return d.to(dtype or g.dtype).to(torch.float64)


def _metric(g, name, dtype, device):
    a = g.arrays[name]
    if a.dtype != dtype or a.device != device:
        a = a.to(device=device, dtype=dtype)
    return a.contiguous()


class AdvectionTimescalePlan:
    """cell_advection_timescale(u, v, w) with its arguments built once: `plan()` issues one tpg_cell_advection_timescale call on torch's
    current stream and allocates nothing (usable inside torch.cuda.graph); `plan.result()` synchronises and returns the float."""

    def __init__(self, u, v, w, not_immersed=True):
        for f, loc, name in ((u, (Face, Center, Center), "u"), (v, (Center, Face, Center), "v"), (w, (Center, Center, Face), "w")):
            if not isinstance(f, Field) or f.loc != loc:
                raise TypeError(f"cell_advection_timescale: {name} must be a Field at ({', '.join(L.__name__ for L in loc)})")
            if f.grid is not u.grid:
                raise ValueError("cell_advection_timescale: u, v and w must live on one grid")
            if f.z_window is not None:
                raise NotImplementedError("cell_advection_timescale: z-windowed fields are not handled")
            if f.data.dtype != u.data.dtype or f.data.device != u.data.device:
                raise ValueError("cell_advection_timescale: u, v and w must share one element type and device")
        if not is_tripolar(u.grid):
            raise TypeError("cell_advection_timescale: the fields' grid must be a TripolarGrid")
        g = _bare(u.grid)
        dtype, device = u.data.dtype, u.data.device
        lib = _lib.lib()
        geom = (u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz)
        counts = getattr(u.grid, "column_counts", None) if not_immersed else None
        ncc = None if counts is None else counts["cc"]
        with torch.cuda.device(device):
            dx, dy = _metric(g, "dx_fc", dtype, device), _metric(g, "dy_cf", dtype, device)
            dz = _grid_table(g, "_z_face_spacings", z_face_spacings, dtype, device)
            self._out = torch.empty(1, dtype=torch.float64, device=device)
            ws = _workspace(lib, 1, geom, device)
        self._held = [u.data, v.data, w.data, dx, dy, dz, ncc, ws]
        args = (u.data.data_ptr(), v.data.data_ptr(), w.data.data_ptr(), dx.data_ptr(), dy.data_ptr(), dz.data_ptr(),
                None if ncc is None else ncc.data_ptr(), self._out.data_ptr(), ws.data_ptr(), ws.numel() * 8, *geom, _lib.ft_of(dtype))
        self._steps = [(device, [(lib.tpg_cell_advection_timescale, args)])]

    def __call__(self):
        for device, calls in self._steps:
            _run(device, calls)
        return self

    def result(self):
        return self._out.item()


def advection_timescale_plan(u, v, w, not_immersed=True):
    return AdvectionTimescalePlan(u, v, w, not_immersed)


def cell_advection_timescale(u, v, w, not_immersed=True):
    """Oceananigans' cell_advection_timescale [recalled; parity unpinned]: the minimum over the interior cells of
        1 / (|u| / Δxᶠᶜᵃ + |v| / Δyᶜᶠᵃ + |w[k]| / Δzᵃᵃᶠ[k]),
    every operation in the fields' type, left to right; NaN if any cell's value is NaN, +inf if the velocities vanish.  u, v, w: Fields at
    (Face, Center, Center), (Center, Face, Center), (Center, Center, Face) of one grid.  On an ImmersedBoundaryGrid with `not_immersed` the
    immersed cells (k <= the (Center, Center) column count) are left out.  A cell whose spacing AND velocity are zero gives 0 / 0 = NaN, as the
    rule says (Δx vanishes where a node sits on a grid pole: such cells belong under the bottom height, as in the reference's examples).
    Returns a float.  On a latitude-band grid: the band's own rows (the cross-rank MIN is the host's)."""
    return AdvectionTimescalePlan(u, v, w, not_immersed)().result()


class TimeStepWizard:
    """TimeStepWizard(cfl = 0.2, max_change = 1.1, min_change = 0.5, max_dt = Inf, min_dt = 0) [recalled: Oceananigans' wizard, its
    new_time_step]: host arithmetic only.
        new = min(max_change * old, cfl * tau);  new = max(min_change * old, new);  new = clamp(new, min_dt, max_dt)
    A NaN timescale gives a NaN step (Julia's min / max propagate it)."""

    def __init__(self, cfl=0.2, max_change=1.1, min_change=0.5, max_dt=math.inf, min_dt=0.0):
        self.cfl, self.max_change, self.min_change, self.max_dt, self.min_dt = cfl, max_change, min_change, max_dt, min_dt

    def new_time_step(self, old_dt, tau):
        if math.isnan(tau) or math.isnan(old_dt):
            return math.nan
        new = min(self.max_change * old_dt, self.cfl * tau)
        new = max(self.min_change * old_dt, new)
        return min(max(new, self.min_dt), self.max_dt)

    def __call__(self, old_dt, u, v, w):
        """the step after `old_dt` for the velocities (u, v, w): new_time_step(old_dt, cell_advection_timescale(u, v, w))"""
        return self.new_time_step(old_dt, cell_advection_timescale(u, v, w))

    def __repr__(self):
        return (f"TimeStepWizard(cfl={self.cfl}, max_change={self.max_change}, min_change={self.min_change}, "
                f"max_dt={self.max_dt}, min_dt={self.min_dt})")


# -------------------------------------------------------------------------------------------------
# grid reductions
# -------------------------------------------------------------------------------------------------
def _metric_extrema(grid, names):
    """(min, max, max|.|) over the interior of the grid's padded 2-D arrays `names`: one tpg_field_extrema call with Nz = 1, Hz = 0"""
    g = _bare(grid)
    tensors = [g.arrays[n] for n in names]
    held = []
    call, out = _extrema_call(_lib.lib(), tensors, (g.Nx, g.Ny, 1, g.Hx, g.Hy, 0), None, None, held)
    _run(tensors[0].device, [call])
    return _triples(out)


def _suffix(LX, LY, what):
    for L in (LX, LY):
        if L is not Center and L is not Face:
            raise TypeError(f"{what}: locations must be Center or Face")
    return ("f" if LX is Face else "c") + ("f" if LY is Face else "c")


def minimum_xspacing(grid, LX=Center, LY=Center):
    """minimum_xspacing(grid, LX, LY): the minimum of Δx at (LX, LY) over the interior i = 1..Nx, j = 1..Ny (a band grid: its own rows)"""
    return _metric_extrema(grid, ["dx_" + _suffix(LX, LY, "minimum_xspacing")])[0][0]


def minimum_yspacing(grid, LX=Center, LY=Center):
    """minimum_yspacing(grid, LX, LY): the minimum of Δy at (LX, LY) over the interior i = 1..Nx, j = 1..Ny (a band grid: its own rows)"""
    return _metric_extrema(grid, ["dy_" + _suffix(LX, LY, "minimum_yspacing")])[0][0]


def grid_summary(grid):
    """The numbers that the `show` of a TripolarGrid prints, as a dict:
        center            (λᶠᶠᵃ, φᶠᶠᵃ) at [Nx÷2+1, Ny÷2+1]
        longitude_extent  rad2deg(Σᵢ Δxᶜᶠᵃ[1:Nx, Ny÷2]) / R          latitude_extent  rad2deg(Σⱼ Δyᶠᶜᵃ[Ny÷2+1, 1:Ny]) / R
        min_dlambda, max_dlambda   rad2deg(min / max of Δxᶠᶠᵃ over the interior) / R
        min_dphi, max_dphi         rad2deg(min / max of Δyᶠᶠᵃ over the interior) / R
    The identification of each printed number with an array reduction is EMPIRICAL (found by matching the
    reference's README transcript to 6 digits), not read from Oceananigans' source.  The four extrema are one tpg_field_extrema call on the
    padded metric arrays; the two extents are sums of one row / one column (a torch sum of the slice: no hot path).  On a latitude-band
    grid everything refers to the band's own rows."""
    g = _bare(grid)
    Nx, Ny, Hx, Hy, R = g.Nx, g.Ny, g.Hx, g.Hy, g.radius
    (dx_min, dx_max, _), (dy_min, dy_max, _) = _metric_extrema(g, ["dx_ff", "dy_ff"])
    j0, i0 = Hy + Ny // 2, Hx + Nx // 2                            # 0-based parent indices of [Nx÷2+1, Ny÷2+1]
    lon = g.arrays["dx_cf"][Hy + Ny // 2 - 1, Hx:Hx + Nx].to(torch.float64).sum().item()
    lat = g.arrays["dy_fc"][Hy:Hy + Ny, Hx + Ny // 2].to(torch.float64).sum().item()
    deg = lambda x: math.degrees(x) / R
    return {"center": (g.arrays["lambda_ff"][j0, i0].item(), g.arrays["phi_ff"][j0, i0].item()),
            "longitude_extent": deg(lon), "latitude_extent": deg(lat),
            "min_dlambda": deg(dx_min), "max_dlambda": deg(dx_max), "min_dphi": deg(dy_min), "max_dphi": deg(dy_max)}


def _sig(x, n=6):
    return str(float(f"{x:.{n}g}"))


def summary(grid):
    """The five lines under the header of a TripolarGrid's `show` (the reference's README.md:55-59), built from grid_summary: 6 significant
    digits, φ of the centre to 4 decimals.  `repr(grid)` stays the one-line header."""
    g = _bare(grid)
    s = grid_summary(g)
    tx, ty, tz = (t.__name__.replace("Topology", "") for t in g.topology)
    zz = _z_spec_values(g)
    z0, z1 = float(zz[0]), float(zz[-1])
    zline = (f"regularly spaced with Δz={_sig((z1 - z0) / g.Nz)}" if len(zz) == 2 else
             f"variably spaced with min(Δz)={_sig(min(b - a for a, b in zip(zz, zz[1:])))}, max(Δz)={_sig(max(b - a for a, b in zip(zz, zz[1:])))}")
    lon = f"├── longitude: {tx}  extent {_sig(s['longitude_extent'])} degrees"
    lat = f"├── latitude:  {ty}  extent {_sig(s['latitude_extent'])} degrees"
    zl = f"└── z:         {tz}  z ∈ [{z0}, {z1}]"
    width = max(len(lon), len(lat), len(zl)) + 1
    return "\n".join([
        repr(g),
        f"├── centered at (λ, φ) = ({_sig(s['center'][0])}, {round(s['center'][1], 4)})",
        f"{lon:<{width}}variably spaced with min(Δλ)={_sig(s['min_dlambda'])}, max(Δλ)={_sig(s['max_dlambda'])}",
        f"{lat:<{width}}variably spaced with min(Δφ)={_sig(s['min_dphi'])}, max(Δφ)={_sig(s['max_dphi'])}",
        f"{zl:<{width}}{zline}"])
