"""What the operator modules share (operators.py, continuity.py, barotropic.py, free_surface.py): the plan that issues ONE C call of an
operator library with its arguments built once, the host checks of the fields of a call, and the Field that remembers its plan.  A module
keeps what is its own: which fields and tables go into the call, and the refusals only it has.  A new operator starts from here."""
import torch

from . import _lib
from .fields import Field, HaloFillPlan
from .grids import is_tripolar


def _loc_names(loc):
    return ", ".join("Nothing" if L is None else L.__name__ for L in loc)


def _ptr(x):
    """the address of a Field's tensor or of a tensor (a tensor's `data` is the tensor); None stays None: a null pointer of the call"""
    return None if x is None else x.data.data_ptr()


def _require(f, name, loc, what):
    if not isinstance(f, Field) or f.loc != loc:
        raise TypeError(f"{what}: {name} must be a Field at ({_loc_names(loc)})")


def _refuse_window(f, what):
    if f.z_window is not None:
        raise NotImplementedError(f"{what}: z-windowed fields are not handled")


def _check_fields(fields, what, group, *, optional=(), type_group=None, grid_note=""):
    """`fields`: the ordered {name: (field, location)} of one call of `what`; the names in `optional` may be None.  Every field given is a
    Field at its location, on the grid of the first, not z-windowed, of the first's element type and device; that grid is a TripolarGrid.
    `group` words the fields in the messages (`type_group`: in the element-type message, if it differs).  Returns the first field given."""
    first = None
    for name, (f, loc) in fields.items():
        if f is None and name in optional:
            continue
        _require(f, name, loc, what)
        first = f if first is None else first
        if f.grid is not first.grid:
            raise ValueError(f"{what}: {group} must live on one grid{grid_note}")
        _refuse_window(f, what)
        if f.data.dtype != first.data.dtype or f.data.device != first.data.device:
            raise ValueError(f"{what}: {type_group or group} must share one element type and device")
    if first is not None and not is_tripolar(first.grid):
        raise TypeError(f"{what}: the fields' grid must be a TripolarGrid")
    return first


class OperatorPlan:
    """One C call with its arguments built once.  `plan()` runs the plans in `before`, issues `fn(*args, stream)` on torch's current stream
    of `device`, passes the status to `check` (the checker of fn's library) and runs one HaloFillPlan of those `outputs` that have
    conditions.  It allocates nothing.  `_call` is (fn, args); `_held` keeps every tensor whose address is in args alive."""

    def _set_call(self, fn, args, check, device, held, outputs=(), before=()):
        self._call, self._check, self._device, self._held, self._before = (fn, args), check, device, held, tuple(before)
        outs = [f for f in outputs if f is not None and f.boundary_conditions is not None]
        self._fill = HaloFillPlan(outs) if outs else None

    def __call__(self):
        for plan in self._before:
            plan()
        fn, args = self._call
        with torch.cuda.device(self._device):
            self._check(fn(*args, _lib.current_stream_ptr(self._device)))
        if self._fill is not None:
            self._fill()
        return self


def _remembering_field(loc, grid, name, plan_of):
    """A Field at `loc` that remembers how it is computed: `plan_of(twin)` builds its plan, which compute_(field) runs.  Nothing is computed
    here (the field holds zeros).  The plan works on a second Field object over the same tensor, so that the returned field and its plan
    form no reference cycle (a cycle would keep a multi-GB tensor alive until the cycle collector runs)."""
    field = Field(loc, grid, name=name)
    twin = Field(loc, grid, data=field.data, boundary_conditions=field.boundary_conditions, name=name)
    field.operand_plan = plan_of(twin)
    return field
