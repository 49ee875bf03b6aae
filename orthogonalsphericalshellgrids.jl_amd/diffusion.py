"""The explicit diffusive tendency of a hydrostatic model on a TripolarGrid with its top and bottom boundary fluxes: what lets anything act
on the ocean from outside.  A field's `FluxBoundaryCondition(q)` on its top or bottom side enters HERE (its halo is a no-flux mirror whatever
q is: boundary_conditions.py), as Oceananigans' apply_z_bcs! puts it into the explicit tendency and not into the implicit step
(vertical_diffusion.py): wind stress on u and v, surface heat and freshwater fluxes, a bottom stress.  With it come the explicit horizontal
diffusion of the tracers, `HorizontalScalarDiffusivity(kappa=...)`, and the explicit form of `VerticalScalarDiffusivity`.

Everything numeric is tpg_diffusive_tendency (libtripolar_hip_diffusion.so): one C call per 16 fields at ONE horizontal location, Center in
z.  THE RULE is written out once, in csrc/staged/tripolar_hip_diffusion.h [recalled: Oceananigans' diffusive_flux_x/y/z, div_dot_q,
apply_z_bcs!, conditional_flux with immersed_peripheral_node; parity unpinned, like every operator here].  On an ImmersedBoundaryGrid the
horizontal faces between wet and dry cells are CLOSED (a wet cell beside land does not diffuse into it: masking the underlying grid's
operator would not do), the bottom flux enters the lowest wet cell of each column, and the cells under the bottom get 0.

The library is STAGED beside the table of _lib.LIBRARIES, whose size is pinned: this module binds it itself with _lib._load, holds its
signature table and DIFFUSION_LIB_PATH (which a caller may assign before the first load), and fails as loudly when the file is missing.

Records: HorizontalScalarDiffusivity(nu, kappa); vertical_diffusion.py's VerticalScalarDiffusivity with ExplicitTimeDiscretization().  The
refusals of vertical_diffusion.refuse_closure still say that the explicit tendency is not built: its messages are pinned and out of date.

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
import ctypes as C
import numbers
import os
from collections.abc import Mapping
from dataclasses import dataclass

import torch

from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _loc_names, _ptr
from .boundary_conditions import Center, Face, is_flux
from .fields import Field
from .reductions import _bare, _grid_table, _metric, z_all_face_spacings, z_center_spacings
from .time_stepping import _on_device
from .vertical_diffusion import ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization, VerticalScalarDiffusivity

TPG_DIFFUSION_HORIZONTAL, TPG_DIFFUSION_VERTICAL = 1, 2                         # bits of `terms` of tpg_diffusive_tendency
TPG_DIFFUSION_ADD, TPG_DIFFUSION_WRITE = 0, 1                                   # its `mode`
TPG_DIFFUSION_KAPPA_CONSTANT, TPG_DIFFUSION_KAPPA_PROFILE, TPG_DIFFUSION_KAPPA_FIELD = 0, 1, 2      # its `kappa_z_form`

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
# every symbol csrc/staged/tripolar_hip_diffusion.h declares, (restype, argtypes)
DIFFUSION_SIGNATURES = {
    "tpg_diffusion_last_error": (C.c_char_p, []),
    "tpg_diffusive_tendency": (_i, [C.POINTER(_vp)] * 2 + [_i] * 3 + [_d, _vp, _d, _i] + [C.POINTER(_vp)] * 2 + [_vp] * 8 + [_d, _vp, _vp, _i]
                               + [_i] * 6 + [_i, _vp]),
}
DIFFUSION_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtripolar_hip_diffusion.so")
_diffusion = None

BUILT = ("HorizontalScalarDiffusivity(kappa=number) on fields at (Center, Center, Center), VerticalScalarDiffusivity("
         "ExplicitTimeDiscretization(), nu, kappa) with a number, Nz + 1 face values or a Field at the fields' horizontal location and Face "
         "in z, and the top and bottom FluxBoundaryCondition of every field are built")
_MODES = {"add": TPG_DIFFUSION_ADD, "write": TPG_DIFFUSION_WRITE}


def diffusion_lib():
    """Load the library at DIFFUSION_LIB_PATH (once); ImportError if it has not been built."""
    global _diffusion
    if _diffusion is None:
        _diffusion = _lib._load(DIFFUSION_LIB_PATH, DIFFUSION_SIGNATURES)
    return _diffusion


def check_diffusion(status):
    if status != 0:
        raise _lib.TripolarHipError(status, diffusion_lib().tpg_diffusion_last_error().decode("utf-8", "replace"))


@dataclass(frozen=True)
class HorizontalScalarDiffusivity:
    """Oceananigans' `HorizontalScalarDiffusivity(; ν, κ)`: a plain record.  `kappa`: the horizontal diffusivity of the tracers, a number.
    A non-zero `nu` is refused where the record is consumed: horizontal viscosity in Oceananigans' divergence-vorticity form is not built."""
    nu: object = 0.0
    kappa: object = 0.0


def _horizontal_kappa(closure, what):
    """the number kappa_h of `horizontal`: None (no horizontal group), a HorizontalScalarDiffusivity or a bare number"""
    if closure is None:
        return None
    if isinstance(closure, HorizontalScalarDiffusivity):
        if not isinstance(closure.nu, numbers.Real) or float(closure.nu) != 0.0:
            raise NotImplementedError(f"{what}: HorizontalScalarDiffusivity(nu={closure.nu!r}): horizontal viscosity in Oceananigans' "
                                      f"divergence-vorticity form is not built ({BUILT})")
        closure = closure.kappa
    if isinstance(closure, numbers.Real) and not isinstance(closure, bool):
        return float(closure)
    if isinstance(closure, (str, Mapping)) or torch.is_tensor(closure) or isinstance(closure, Field):
        raise NotImplementedError(f"{what}: a horizontal diffusivity {closure!r} is not built: kappa_h is one number ({BUILT})")
    raise NotImplementedError(f"{what}: {type(closure).__name__} is not built as a horizontal closure ({BUILT})")


def _vertical_kappa(closure, loc, what):
    """the kappa_z of `vertical` for fields at `loc`: None (no interior vertical fluxes), a VerticalScalarDiffusivity with the explicit
    discretization (nu for u and v, kappa for everything at (Center, Center)), or a bare number, profile or Field"""
    if closure is None:
        return None
    if isinstance(closure, VerticalScalarDiffusivity):
        disc = closure.time_discretization
        if isinstance(disc, VerticallyImplicitTimeDiscretization):
            raise NotImplementedError(f"{what}: VerticallyImplicitTimeDiscretization is the implicit step's (implicit_step_plan), not the "
                                      f"explicit tendency's ({BUILT})")
        if not isinstance(disc, ExplicitTimeDiscretization):
            raise NotImplementedError(f"{what}: the time discretization {disc!r} is not built ({BUILT})")
        k = closure.kappa if loc[:2] == (Center, Center) else closure.nu
        if isinstance(k, Mapping):
            raise TypeError(f"{what}: the fields of one call share one kappa_z: pass one value, and make one plan per diffusivity")
        return k
    if isinstance(closure, (numbers.Real, Field)) and not isinstance(closure, bool) or torch.is_tensor(closure):
        return closure
    if isinstance(closure, (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization)):
        raise NotImplementedError(f"{what}: {type(closure).__name__} is a time discretization, not a closure ({BUILT})")
    raise NotImplementedError(f"{what}: {type(closure).__name__} is not built ({BUILT})")


def _count_key(loc):
    return ("f" if loc[0] is Face else "c") + ("f" if loc[1] is Face else "c")


def _flux_plane(value, f, side, what, held):
    """the padded (Ny + 2Hy, Nx + 2Hx) device plane of one field's flux through `side`, or None: a number gives a constant plane made here,
    once; a plane or a reduced Field at the field's horizontal location is read at call time"""
    if value is None:
        return None
    dtype, device = f.data.dtype, f.data.device
    shape = (f.Ny + 2 * f.Hy, f.Nx + 2 * f.Hx)
    if isinstance(value, Field):
        if value.loc != (f.loc[0], f.loc[1], None) or value.grid is not f.grid or value.data.dtype != dtype:
            raise ValueError(f"{what}: a {side} flux Field must be a reduced Field(({_loc_names(f.loc[:2])}, Nothing)) on the fields' grid and of "
                             f"their type (it is at ({_loc_names(value.loc)}))")
        plane = value.data.view(value.data.shape[-2:])
    elif isinstance(value, numbers.Real) and not isinstance(value, bool) or (torch.is_tensor(value) and value.dim() == 0):
        with _on_device(device):
            plane = torch.full(shape, float(value), dtype=dtype, device=device)
    elif torch.is_tensor(value) and tuple(value.shape) == shape and value.is_contiguous() and value.device == device and value.dtype == dtype:
        plane = value
    else:
        got = f"a {tuple(value.shape)} tensor of {value.dtype} on {value.device}" if torch.is_tensor(value) else repr(value)
        raise ValueError(f"{what}: a {side} flux must be None, a number, a contiguous {shape} tensor of {dtype} on {device} or a reduced Field "
                         f"at the fields' horizontal location (it is {got})")
    held.append(plane)
    return plane


def _fluxes(spec, fields, side, what, held):
    """the planes of the fields' fluxes through `side` (None each where there is none), or None if no field has one"""
    if isinstance(spec, str):
        if spec != "from_fields":
            raise ValueError(f"{what}: {side}_flux {spec!r} is not 'from_fields', None, a number, a plane, a reduced Field or a list of those")
        values = []
        for f in fields:                                          # a side that is not Flux contributes nothing, and is no error
            bc = None if f.boundary_conditions is None else getattr(f.boundary_conditions, side)
            values.append(bc.condition if is_flux(bc) else None)
    elif isinstance(spec, (list, tuple)):
        if len(spec) != len(fields):
            raise TypeError(f"{what}: {side}_flux is a list of one entry per field ({len(spec)} for {len(fields)} fields)")
        values = list(spec)
    else:
        values = [spec] * len(fields)
    planes = [_flux_plane(v, f, side, what, held) for v, f in zip(values, fields)]
    return planes if any(p is not None for p in planes) else None


class DiffusiveTendencyPlan(OperatorPlan):
    """diffusive_tendency(fields, out=G, ...) with the arguments built once: `plan()` issues ONE tpg_diffusive_tendency call per 16 fields on
    torch's current stream.  It allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.
    `fields`: a Field or a list of Fields at ONE horizontal location, Center in z, on one grid; `G`: their tendencies, there too.
    `horizontal`: None, a HorizontalScalarDiffusivity or a number -- fields at (Center, Center) only, whose halos the caller HAS FILLED.
    `vertical`: None, VerticalScalarDiffusivity(ExplicitTimeDiscretization(), nu, kappa) (nu for u and v, kappa elsewhere), or a number,
    Nz + 1 face values or a Field at (the fields' horizontal location, Face).  `top_flux`, `bottom_flux`: "from_fields" (each field's own
    FluxBoundaryCondition(q) of that side; any other class of condition contributes nothing), None, a number (a constant plane made here,
    once), a padded (Ny + 2Hy, Nx + 2Hx) device plane or a reduced Field (read at call time), or a list of those, one per field.  A positive
    flux points up: a positive top flux removes the quantity, a positive bottom flux adds it.  `mode`: "add" (G += D: after the advection
    and hydrostatic calls, before AB2) or "write".  On an ImmersedBoundaryGrid, with `mask_immersed` the count plane of the fields' location
    and the value 0 go into the call, and with `close_immersed_faces` the grid's filled bottom height and z centres, so that the faces
    between wet and dry cells carry no flux.  The plan holds every tensor: rebuild it if a field's `data` is replaced."""

    def __init__(self, fields, G, *, horizontal=None, vertical=None, top_flux="from_fields", bottom_flux="from_fields", mode="add",
                 mask_immersed=True, close_immersed_faces=True, what="diffusive_tendency_plan"):
        fields = [fields] if isinstance(fields, Field) else list(fields)
        G = [G] if isinstance(G, Field) else list(G)
        if not fields:
            raise TypeError(f"{what}: no fields")
        if len(fields) != len(G):
            raise TypeError(f"{what}: fields and G are lists of one length ({len(fields)}, {len(G)})")
        for q, f in enumerate(fields):
            if not isinstance(f, Field):
                raise TypeError(f"{what}: field {q} must be a Field")
        loc = fields[0].loc
        if loc[2] is not Center or None in loc[:2]:
            raise TypeError(f"{what}: the fields must be Center in z at a (Center or Face, Center or Face) location (field 0 at ({_loc_names(loc)}))")
        for q, f in enumerate(fields):
            if f.loc != loc:
                raise ValueError(f"{what}: the fields of one call share the metrics and the count plane, so one location: field {q} at "
                                 f"({_loc_names(f.loc)}) against ({_loc_names(loc)}); use one call per location")
        if mode not in _MODES:
            raise ValueError(f"{what}: mode {mode!r} is not one of 'add' and 'write'")
        kh = _horizontal_kappa(horizontal, what)
        kz = _vertical_kappa(vertical, loc, what)
        if kh is not None and loc[:2] != (Center, Center):
            raise NotImplementedError(f"{what}: the horizontal group is defined for fields at (Center, Center, Center) only (they are at "
                                      f"({_loc_names(loc)})): horizontal viscosity is not built ({BUILT})")
        names = {}
        for q, (f, g) in enumerate(zip(fields, G)):
            names.update({f"field {q}": (f, loc), f"G of field {q}": (g, loc)})
        kloc = (loc[0], loc[1], Face)
        if isinstance(kz, Field):
            if kz.loc != kloc:
                raise TypeError(f"{what}: a kappa Field must be at ({_loc_names(kloc)}), the fields' horizontal location and Face in z (it is at "
                                f"({_loc_names(kz.loc)}))")
            names["kappa"] = (kz, kloc)
        first = _check_fields(names, what, "the fields, their tendencies and kappa")
        for q, g in enumerate(G):
            for r, f in enumerate(fields):
                if g is f or g.data.data_ptr() == f.data.data_ptr():
                    raise ValueError(f"{what}: G of field {q} is field {r} itself (every node reads its neighbours while they are written)")
            for r in range(q):
                if g is G[r] or g.data.data_ptr() == G[r].data.data_ptr():
                    raise ValueError(f"{what}: G of field {q} and G of field {r} are one field")
        if kh is not None and (first.Hx < 1 or first.Hy < 1):
            raise ValueError(f"{what}: the horizontal group reads one cell beyond the interior west, east, south and north: Hx and Hy must be at "
                             f"least 1 (halo ({first.Hx}, {first.Hy}, {first.Hz}))")
        g = _bare(first.grid)
        if g.global_size and g.Ny != g.global_size[1]:
            raise NotImplementedError(f"{what}: latitude-band grids are not handled: the rows 0 and Ny + 1 of a band are exchanged halo rows, and "
                                      "the band path of the diffusive tendency is not tested yet")
        dtype, device = first.data.dtype, first.data.device
        Nz = first.Nz
        value, form, ktensor = 0.0, TPG_DIFFUSION_KAPPA_CONSTANT, None
        if isinstance(kz, Field):
            form, ktensor = TPG_DIFFUSION_KAPPA_FIELD, kz.data
        elif torch.is_tensor(kz) and kz.dim() > 0:
            if tuple(kz.shape) != (Nz + 1,) or kz.dtype != dtype or kz.device != device or not kz.is_contiguous():
                raise ValueError(f"{what}: a kappa profile must be a contiguous tensor of Nz + 1 = {Nz + 1} face values in the fields' element type "
                                 f"and device (it is {tuple(kz.shape)}, {kz.dtype}, {kz.device})")
            form, ktensor = TPG_DIFFUSION_KAPPA_PROFILE, kz
        elif kz is not None:
            value = float(kz)
        held = []
        top = _fluxes(top_flux, fields, "top", what, held)
        bottom = _fluxes(bottom_flux, fields, "bottom", what, held)
        terms = (TPG_DIFFUSION_HORIZONTAL if kh is not None else 0) | (TPG_DIFFUSION_VERTICAL if kz is not None else 0)
        if not terms and top is None and bottom is None:
            raise TypeError(f"{what}: nothing to compute: no horizontal closure, no vertical closure and no field has a top or bottom flux")
        self.fields, self.G, self.horizontal, self.vertical, self.mode, self.terms = fields, G, horizontal, vertical, mode, terms
        self.top_flux, self.bottom_flux = top, bottom
        lib = diffusion_lib()
        counts = getattr(first.grid, "column_counts", None)
        plane = None if counts is None or not mask_immersed else counts[_count_key(loc)]
        h = zc = None
        wall = 1
        with _on_device(device):
            az = _metric(g, "az_" + _count_key(loc), dtype, device)
            metrics = [_metric(g, name, dtype, device) for name in ("dx_fc", "dy_fc", "dx_cf", "dy_cf")] if kh is not None else [None] * 4
            dzc = _grid_table(g, "_z_center_spacings", z_center_spacings, dtype, device)
            dzf = _grid_table(g, "_z_all_face_spacings", z_all_face_spacings, dtype, device) if kz is not None else None
            if counts is not None and close_immersed_faces and kh is not None:
                bottom_field = first.grid.immersed_boundary.bottom_height
                if bottom_field.data.dtype != dtype:
                    raise ValueError(f"{what}: the grid's bottom height is {bottom_field.data.dtype} and the fields are {dtype}: the closed faces are "
                                     "compared in the fields' type")
                h = bottom_field.data.view(bottom_field.data.shape[-2:])
                zc = g.z_centers[g.Hz:g.Hz + g.Nz].to(device=device, dtype=dtype).contiguous()
                arch = g.architecture
                wall = int(not (getattr(arch, "is_distributed", False) and arch.local_rank > 0))     # as the grid built its counts
        shared = [ktensor, *metrics, az, dzc, dzf, plane, h, zc]
        calls = []
        for f0 in range(0, len(fields), _lib.TPG_MAX_FIELDS):      # more than 16 fields go in several calls, as the AB2 step's do
            sl = slice(f0, f0 + _lib.TPG_MAX_FIELDS)
            tables = [_lib.ptr_table([t.data for t in fields[sl]]), _lib.ptr_table([t.data for t in G[sl]])]
            flux = [None if planes is None else (C.c_void_p * len(fields[sl]))(*[_ptr(t) for t in planes[sl]]) for planes in (top, bottom)]
            # a batch whose fields have no flux keeps an (all-null) table: the vertical group is a property of the plan
            calls.append((tables + flux, (*tables, len(fields[sl]), terms, _MODES[mode], 0.0 if kh is None else kh, _ptr(ktensor), value, form,
                                          *flux, *(_ptr(t) for t in metrics), _ptr(az), _ptr(dzc), _ptr(dzf), _ptr(plane), 0.0, _ptr(h), _ptr(zc),
                                          wall, first.Nx, first.Ny, first.Nz, first.Hx, first.Hy, first.Hz, _lib.ft_of(dtype))))
        held += [t.data for t in (*fields, *G)] + [t for t in shared if t is not None] + [c[0] for c in calls]
        before = []
        for _, args in calls[:-1]:
            p = OperatorPlan()
            p._set_call(lib.tpg_diffusive_tendency, args, check_diffusion, device, held)
            before.append(p)
        self._set_call(lib.tpg_diffusive_tendency, calls[-1][1], check_diffusion, device, held, before=before)


def diffusive_tendency_plan(fields, G, *, horizontal=None, vertical=None, top_flux="from_fields", bottom_flux="from_fields", mode="add",
                            mask_immersed=True, close_immersed_faces=True):
    return DiffusiveTendencyPlan(fields, G, horizontal=horizontal, vertical=vertical, top_flux=top_flux, bottom_flux=bottom_flux, mode=mode,
                                 mask_immersed=mask_immersed, close_immersed_faces=close_immersed_faces)


def diffusive_tendency(fields, out=None, *, horizontal=None, vertical=None, top_flux="from_fields", bottom_flux="from_fields", mode=None,
                       mask_immersed=True, close_immersed_faces=True):
    """The explicit diffusive tendencies of `fields` (a Field or a list at one horizontal location, Center in z) with their top and bottom
    boundary fluxes, as a list of Fields there: the rule of tpg_diffusive_tendency on every interior node.  `out`: the fields to add to or
    write into, one per field; None allocates a Field per field and writes.  `mode`: "add" or "write"; None: "add" into a given `out`,
    "write" into a new one.  Returns the list.  Builds a DiffusiveTendencyPlan and runs it once; use diffusive_tendency_plan in a time loop."""
    what = "diffusive_tendency"
    fields = [fields] if isinstance(fields, Field) else list(fields)
    if mode is None:
        mode = "write" if out is None else "add"
    if out is None:
        for q, f in enumerate(fields):
            if not isinstance(f, Field):
                raise TypeError(f"{what}: field {q} must be a Field")
        out = [Field(f.loc, f.grid, name="G") for f in fields]
    plan = DiffusiveTendencyPlan(fields, out, horizontal=horizontal, vertical=vertical, top_flux=top_flux, bottom_flux=bottom_flux, mode=mode,
                                 mask_immersed=mask_immersed, close_immersed_faces=close_immersed_faces, what=what)
    plan()
    return plan.G
