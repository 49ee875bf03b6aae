"""The flux-form advection tendency of the tracers with the scheme of the reference's second driver: examples/distributed_bickley_jet.jl:50
has `tracer_advection = WENO()`, fifth-order WENO in ALL THREE directions.  The tracer at an x-, y- or z-face is the WENO reconstruction
biased against the flow; the result is the Gⁿ of the AB2 step of the tracers, as weno_tracer_advection_tendency's (weno.py: WENO in x and
y, the centred mean in z) is.

Everything numeric is tpg_weno_xyz_tracer_advection_tendency (libtripolar_hip_weno_xyz.so).  THE RULE is written out once, in
include/tripolar_hip_weno_xyz.h: x and y are include/tripolar_hip_weno.h's; a z-face f = 1..Nz+1 takes, by its distance
min(f - 1, Nz + 1 - f) from the nearer wall and whichever way the flow goes, the centred mean (0: the bottom and the surface), the upwind
cell (1), the third-order face value R3 (2) or the fifth-order R5 (3 and more) -- in the fields' type T, in exactly that order, with no
contraction, every operation one correctly rounded IEEE operation [recalled: Oceananigans' WENO() = FluxFormAdvection(WENO(order = 5) x3)
on a z-Bounded grid; parity unpinned, like every operator here].  With Nz = 1 it is weno_tracer_advection_tendency bit for bit.  The rule
reads c[-2..Nx+3, j, k], c[i, -2..Ny+3, k] and c[i, j, 0..Nz+1]: no face of a reduced order reads a z-halo plane, so the halo is at least
(3, 3, 1) as there, and the halos of c, u and v are the caller's to fill first; w is what compute_w_from_continuity writes.  Only interior
cells of G are written.  On an ImmersedBoundaryGrid the nodes k <= n_cc[i,j] of G get 0 inside the same launch, and everything is computed
unmasked.

Stays out: Oceananigans' drop of the reconstruction order beside the south wall and beside immersed nodes, in all three
directions now (faces above an immersed bottom take the full order on the masked cells below them); stretched-grid coefficients; other
orders; latitude bands; the Julia hooks.

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
from . import weno
from .advection import _TracerTendencyPlan, _tendency_fields
from .weno import WENO, FluxFormAdvection

BUILT = WENO(order=5)
_ACCEPTED = (BUILT, FluxFormAdvection(BUILT, BUILT, BUILT))
_BUILT_NAME = "WENO(order=5), the same as FluxFormAdvection(WENO(order=5), WENO(order=5), WENO(order=5))"


class WenoXyzTracerAdvectionPlan(_TracerTendencyPlan):
    """weno_xyz_tracer_advection_tendency(tracers, u, v, w, out=G) with the arguments built once: `plan()` issues ONE
    tpg_weno_xyz_tracer_advection_tendency call per 16 tracers on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of
    those G that have conditions.  It allocates nothing when called and is a single chain of launches, so it replays inside
    torch.cuda.graph.  On an ImmersedBoundaryGrid with `mask_immersed` the (Center, Center) count plane and the value 0 go into the call.
    The plan holds the tensors of the tracers, u, v, w and G, the metric arrays, the spacings and the count plane: rebuild it if a field's
    `data` is replaced."""
    _HALO = (3, 3, 1)
    _HALO_RULE = ("the rule reads three cells beyond the interior in x and y and, in z, the planes 0 and Nz + 1 only (the faces beside a wall "
                  "drop their order): the halo must be at least (3, 3, 1)")
    _BAND_ROWS = "the rows Ny + 1 .. Ny + 3 of a band are exchanged halo rows"
    _LIBRARY = ("weno_xyz_lib", "check_weno_xyz", "tpg_weno_xyz_tracer_advection_tendency")

    def __init__(self, tracers, u, v, w, G, *, scheme=BUILT, mask_immersed=True, fill_halos=False, what="weno_xyz_tracer_advection_plan"):
        super().__init__(tracers, u, v, w, G, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)

    @staticmethod
    def _refuse(scheme, what):
        if isinstance(scheme, (WENO, FluxFormAdvection)) and scheme in _ACCEPTED:
            return
        elsewhere = " (weno_tracer_advection_tendency has it)" if isinstance(scheme, FluxFormAdvection) and scheme == weno.BUILT else ""
        raise NotImplementedError(f"{what}: advection scheme {scheme!r} is not built{elsewhere} ({_BUILT_NAME} is: WENO of order 5 in x, y and "
                                  "z, the order dropping beside the bottom and the surface)")

    @staticmethod
    def _extra(scheme):
        return ()


def weno_xyz_tracer_advection_plan(tracers, u, v, w, G, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    return WenoXyzTracerAdvectionPlan(tracers, u, v, w, G, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos)


def weno_xyz_tracer_advection_tendency(tracers, u, v, w, out=None, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    """The advective tendencies G = -div(U c) of the `tracers` (a list of Fields at (Center, Center, Center)) as a list of Fields there: the
    rule of tpg_weno_xyz_tracer_advection_tendency (include/tripolar_hip_weno_xyz.h) on every interior node -- fifth-order WENO in x, y and
    z, the order of a z-face dropping beside the bottom and the surface.  `scheme`: WENO(), WENO(order=5) or
    FluxFormAdvection(WENO(), WENO(), WENO()), all the same thing and the only one built.  u at (Face, Center, Center), v at
    (Center, Face, Center), w at (Center, Center, Face) and the tracers live on one TripolarGrid with a halo of at least (3, 3, 1), share
    element type and device, and the tracers, u and v HAVE THEIR HALOS FILLED; w is compute_w_from_continuity's.  `out`: the fields to write
    into, one per tracer; None allocates CenterField(grid) for each.  More than 16 tracers go in several calls.  On an ImmersedBoundaryGrid
    with `mask_immersed` the nodes under the bottom get 0.  Only the interior of each G is written; `fill_halos` then fills those that have
    conditions.  Returns the list.  Builds a WenoXyzTracerAdvectionPlan and runs it once; use weno_xyz_tracer_advection_plan in a time
    loop."""
    tracers = list(tracers)
    out = _tendency_fields(tracers, out, "weno_xyz_tracer_advection_tendency")
    plan = WenoXyzTracerAdvectionPlan(tracers, u, v, w, out, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos,
                                      what="weno_xyz_tracer_advection_tendency")
    plan()
    return plan.G
