"""The flux-form advection tendency of the tracers on a TripolarGrid: what the AB2 step of the tracers (time_stepping.py) consumes as Gⁿ.
Both of the reference's drivers carry a tracer (`tracers = :c`, examples/bickley_jet.jl:48-55); with `buoyancy = nothing`, no closure and no
forcing its only tendency is minus the divergence of its advective flux.  With it a tracer is time-stepped end to end on the device:
tendency -> ab2_step_fields -> halo fill.

Everything numeric is tpg_tracer_advection_tendency (include/tripolar_hip_advection.h, libtripolar_hip_advection.so): one launch over the
interior nodes i = 1..Nx, j = 1..Ny, k = 1..Nz, in the fields' type T, in exactly this order, with no contraction, every operation one
correctly rounded IEEE operation:
    d = dz_c[k]
    Mx[i,j,k] = (dy_fc[i,j] * d) * u[i,j,k]           i = 1..Nx+1     (the continuity's fe / fw, the same bits)
    My[i,j,k] = (dx_cf[i,j] * d) * v[i,j,k]           j = 1..Ny+1
    Mz[i,j,k] =  az_cc[i,j]      * w[i,j,k]           k = 1..Nz+1     (w has Nz+1 levels)
    Fx[i,j,k] = Mx[i,j,k] * (T(0.5) * (c[i-1,j,k] + c[i,j,k]))
    Fy[i,j,k] = My[i,j,k] * (T(0.5) * (c[i,j-1,k] + c[i,j,k]))
    Fz[i,j,k] = Mz[i,j,k] * (T(0.5) * (c[i,j,k-1] + c[i,j,k]))
    V = az_cc[i,j] * d
    G[i,j,k] = -((T(1) / V) * (((Fx[i+1,j,k] - Fx[i,j,k]) + (Fy[i,j+1,k] - Fy[i,j,k])) + (Fz[i,j,k+1] - Fz[i,j,k])))
[recalled: Oceananigans' div_Uc with Centered(order = 2) in all three directions, _advective_tracer_flux_x/y/z, and
hydrostatic_free_surface_tracer_tendency with no diffusion and no forcing; parity unpinned, like every operator here].  Each flux is formed
once; the leading minus is a sign flip; V = 0 divides by it.  The rule reads c[0..Nx+1, j, k], c[i, 0..Ny+1, k], c[i, j, 0..Nz+1] (a
plus-shaped stencil, no corner halo cell), u[1..Nx+1], v[.., 1..Ny+1] and w[.., 1..Nz+1]: every halo is at least 1 wide, and the halos of c, u
and v are the caller's to fill first; w is what compute_w_from_continuity writes.  Only interior cells of G are written.  On an
ImmersedBoundaryGrid the nodes k <= n_cc[i,j] of G get 0 inside the same launch -- what mask_immersed_field leaves on a Center field --
and everything is computed unmasked (with the model's masked velocities the flux through a solid face is already +-0; Oceananigans'
conditional reconstruction beside an immersed node is out of scope).  The plan form holds its tensors: calling it enqueues on
torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _ptr
from .boundary_conditions import Center, Face
from .fields import Field
from .reductions import _bare, _grid_table, _metric, z_center_spacings
from .time_stepping import _on_device

_LOCS = {"c": (Center, Center, Center), "u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}
_SCHEMES = {"centered2": _lib.TPG_ADVECTION_CENTERED2}


def _same(a, b):
    return a is b or a.data is b.data or a.data.data_ptr() == b.data.data_ptr()


class _TracerTendencyPlan(OperatorPlan):
    """The plan of a flux-form tracer tendency, whatever the scheme: the checks of the fields, the metric arrays, one C call per 16 tracers and
    the halo fill of those G that have conditions.  A scheme's class (TracerAdvectionPlan here, WenoTracerAdvectionPlan in weno.py) supplies
    what differs: `_refuse(scheme, what)`, the smallest halo `_HALO` with the sentence `_HALO_RULE` of its refusal, the band refusal's
    `_BAND_ROWS`, `_LIBRARY` (the names in _lib of the loader and the checker, and the C function) and `_extra(scheme)`, the arguments
    between the mask value and Nx."""

    def __init__(self, tracers, u, v, w, G, *, scheme, mask_immersed, fill_halos, what):
        tracers, G = list(tracers), list(G)
        if not tracers:
            raise TypeError(f"{what}: no tracers")
        if len(tracers) != len(G):
            raise TypeError(f"{what}: tracers and G are lists of one length ({len(tracers)}, {len(G)})")
        self._refuse(scheme, what)
        names = {"u": (u, _LOCS["u"]), "v": (v, _LOCS["v"]), "w": (w, _LOCS["w"])}
        for q, (c, g) in enumerate(zip(tracers, G)):
            names.update({f"tracer {q}": (c, _LOCS["c"]), f"G of tracer {q}": (g, _LOCS["c"])})
        first = _check_fields(names, what, "the tracers, their tendencies, u, v and w")
        for q, g in enumerate(G):
            for p, c in enumerate(tracers):
                if _same(g, c):
                    raise ValueError(f"{what}: G of tracer {q} is tracer {p} itself (every node reads its neighbours while they are written)")
            for p in range(q):
                if _same(g, G[p]):
                    raise ValueError(f"{what}: G of tracer {q} and G of tracer {p} are one field")
        if any(h < least for h, least in zip((first.Hx, first.Hy, first.Hz), self._HALO)):
            raise ValueError(f"{what}: {self._HALO_RULE} (halo ({first.Hx}, {first.Hy}, {first.Hz}))")
        g = _bare(first.grid)
        if g.global_size and g.Ny != g.global_size[1]:
            raise NotImplementedError(f"{what}: latitude-band grids are not handled: {self._BAND_ROWS}, and the band path of the tracer "
                                      "tendency is not tested yet")
        self.tracers, self.u, self.v, self.w, self.G, self.scheme = tracers, u, v, w, G, scheme
        dtype, device = u.data.dtype, u.data.device
        load, check, function = self._LIBRARY
        function, check = getattr(getattr(_lib, load)(), function), getattr(_lib, check)
        counts = getattr(first.grid, "column_counts", None) if mask_immersed else None
        ncc = None if counts is None else counts["cc"]
        with _on_device(device):
            dy, dx, az = (_metric(g, name, dtype, device) for name in ("dy_fc", "dx_cf", "az_cc"))
            dz = _grid_table(g, "_z_center_spacings", z_center_spacings, dtype, device)
        shared = [u.data, v.data, w.data, dy, dx, az, dz, ncc]
        tail = (*(_ptr(t) for t in shared), 0.0, *self._extra(scheme), u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz, _lib.ft_of(dtype))
        calls = []
        for f0 in range(0, len(tracers), _lib.TPG_MAX_FIELDS):     # more than 16 tracers go in several calls, as the AB2 step's do
            sl = slice(f0, f0 + _lib.TPG_MAX_FIELDS)
            tables = [_lib.ptr_table([t.data for t in tracers[sl]]), _lib.ptr_table([t.data for t in G[sl]])]
            calls.append((tables, (*tables, len(tracers[sl]), *tail)))
        held = [t.data for t in (*tracers, *G)] + shared + [c[0] for c in calls]
        before = []
        for _, args in calls[:-1]:
            p = OperatorPlan()
            p._set_call(function, args, check, device, held)
            before.append(p)
        self._set_call(function, calls[-1][1], check, device, held, G if fill_halos else (), before=before)


def _tendency_fields(tracers, out, what):
    """the `out` of a one-shot call: as given, or a new Field at (Center, Center, Center) per tracer"""
    if out is not None:
        return out
    for q, c in enumerate(tracers):
        if not isinstance(c, Field) or c.loc != _LOCS["c"]:
            raise TypeError(f"{what}: tracer {q} must be a Field at (Center, Center, Center)")
    return [Field(_LOCS["c"], c.grid, name="G") for c in tracers]


class TracerAdvectionPlan(_TracerTendencyPlan):
    """tracer_advection_tendency(tracers, u, v, w, out=G) with the arguments built once: `plan()` issues ONE tpg_tracer_advection_tendency
    call per 16 tracers on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of those G that have conditions.  It
    allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  On an ImmersedBoundaryGrid with
    `mask_immersed` the (Center, Center) count plane and the value 0 go into the call.  The plan holds the tensors of the tracers, u, v, w and
    G, the metric arrays, the spacings and the count plane: rebuild it if a field's `data` is replaced."""
    _HALO = (1, 1, 1)
    _HALO_RULE = "the rule reads one cell beyond the interior on every side: every halo must be at least 1"
    _BAND_ROWS = "the row Ny + 1 of a band is the exchanged halo row"
    _LIBRARY = ("advection_lib", "check_advection", "tpg_tracer_advection_tendency")

    def __init__(self, tracers, u, v, w, G, *, scheme="centered2", mask_immersed=True, fill_halos=False, what="tracer_advection_plan"):
        super().__init__(tracers, u, v, w, G, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)

    @staticmethod
    def _refuse(scheme, what):
        if scheme not in _SCHEMES:
            raise NotImplementedError(f"{what}: advection scheme {scheme!r} is not built ('centered2' is; upwind and WENO are not)")

    @staticmethod
    def _extra(scheme):
        return (_SCHEMES[scheme],)


def tracer_advection_plan(tracers, u, v, w, G, *, scheme="centered2", mask_immersed=True, fill_halos=False):
    return TracerAdvectionPlan(tracers, u, v, w, G, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos)


def tracer_advection_tendency(tracers, u, v, w, out=None, *, scheme="centered2", mask_immersed=True, fill_halos=False):
    """The advective tendencies G = -div(U c) of the `tracers` (a list of Fields at (Center, Center, Center)) as a list of Fields there: the
    rule of tpg_tracer_advection_tendency on every interior node, second-order centered.  u at (Face, Center, Center), v at
    (Center, Face, Center), w at (Center, Center, Face) and the tracers live on one TripolarGrid, share element type and device, and the
    tracers, u and v HAVE THEIR HALOS FILLED; w is compute_w_from_continuity's.  `out`: the fields to write into, one per tracer; None
    allocates CenterField(grid) for each.  More than 16 tracers go in several calls.  On an ImmersedBoundaryGrid with `mask_immersed` the
    nodes under the bottom get 0.  Only the interior of each G is written; `fill_halos` then fills those that have conditions.  Returns the
    list.  Builds a TracerAdvectionPlan and runs it once; use tracer_advection_plan in a time loop."""
    tracers = list(tracers)
    out = _tendency_fields(tracers, out, "tracer_advection_tendency")
    plan = TracerAdvectionPlan(tracers, u, v, w, out, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos,
                               what="tracer_advection_tendency")
    plan()
    return plan.G
