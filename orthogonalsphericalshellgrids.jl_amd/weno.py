"""The flux-form advection tendency of the tracers with the scheme the reference's drivers build: examples/bickley_jet.jl:48 has
`FluxFormAdvection(WENO(; order = 5), WENO(; order = 5), Centered())`, examples/distributed_bickley_jet.jl:50 `WENO()`.  The tracer at an
x- or y-face is the fifth-order WENO reconstruction biased against the flow, at a z-face the centred mean; the result is the Gⁿ of the AB2
step of the tracers, as tracer_advection_tendency's (advection.py, second-order centred) is.

Everything numeric is tpg_weno_tracer_advection_tendency (libtripolar_hip_weno.so).  THE RULE is written out once, in
include/tripolar_hip_weno.h: the face value R(q0, q1, q2, q3, q4) (uniform-grid coefficients, Jiang-Shu smoothness indicators, WENO-Z
weights, eps = 1e-8), Fx = Mx * (Mx >= 0 ? R(c[i-3..i+1]) : R(c[i+2..i-2])) and the same in y with My, Fz and the last line those of
tpg_tracer_advection_tendency -- in the fields' type T, in exactly that order, with no contraction, every operation one correctly rounded
IEEE operation [recalled: Oceananigans' FluxFormAdvection(WENO(order = 5), WENO(order = 5), Centered()); parity unpinned, like every
operator here].  The rule reads c[-2..Nx+3, j, k], c[i, -2..Ny+3, k] and c[i, j, 0..Nz+1] (a plus-shaped stencil, no corner halo cell):
the halo is at least (3, 3, 1), and the halos of c, u and v are the caller's to fill first -- the rows Ny+1..Ny+3 are the Zipper's, the
rows -2..0 what the south condition left there; w is what compute_w_from_continuity writes.  Only interior cells of G are written.  On an
ImmersedBoundaryGrid the nodes k <= n_cc[i,j] of G get 0 inside the same launch, and everything is computed unmasked.

Stays out: Oceananigans' drop of the reconstruction order beside the south wall and beside immersed nodes (in both drivers
every row south of -78 degrees and both pole boxes are under the mask, so the rows this touches are masked in the workloads here);
stretched-grid coefficients; other orders; latitude bands; the Julia hooks.  WENO in z is weno_xyz.py's call, not this one's.  The momentum half of the drivers' scheme is weno_momentum.py's.

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
from dataclasses import dataclass

from .advection import _TracerTendencyPlan, _tendency_fields


@dataclass(frozen=True)
class WENO:
    """the reference driver's `WENO(; order = 5)`: a plain record.  WENO() means order 5."""
    order: int = 5


@dataclass(frozen=True)
class Centered:
    """the reference driver's `Centered()`: a plain record, second order"""
    order: int = 2


@dataclass(frozen=True)
class FluxFormAdvection:
    """the reference driver's `FluxFormAdvection(x, y, z)`: one scheme per direction"""
    x: object
    y: object
    z: object


BUILT = FluxFormAdvection(WENO(order=5), WENO(order=5), Centered())
_BUILT_NAME = "FluxFormAdvection(WENO(order=5), WENO(order=5), Centered())"


class WenoTracerAdvectionPlan(_TracerTendencyPlan):
    """weno_tracer_advection_tendency(tracers, u, v, w, out=G) with the arguments built once: `plan()` issues ONE
    tpg_weno_tracer_advection_tendency call per 16 tracers on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of those
    G that have conditions.  It allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  On
    an ImmersedBoundaryGrid with `mask_immersed` the (Center, Center) count plane and the value 0 go into the call.  The plan holds the
    tensors of the tracers, u, v, w and G, the metric arrays, the spacings and the count plane: rebuild it if a field's `data` is replaced."""
    _HALO = (3, 3, 1)
    _HALO_RULE = "the rule reads three cells beyond the interior in x and y and one in z: the halo must be at least (3, 3, 1)"
    _BAND_ROWS = "the rows Ny + 1 .. Ny + 3 of a band are exchanged halo rows"
    _LIBRARY = ("weno_lib", "check_weno", "tpg_weno_tracer_advection_tendency")

    def __init__(self, tracers, u, v, w, G, *, scheme=BUILT, mask_immersed=True, fill_halos=False, what="weno_tracer_advection_plan"):
        super().__init__(tracers, u, v, w, G, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)

    @staticmethod
    def _refuse(scheme, what):
        if not isinstance(scheme, FluxFormAdvection) or scheme != BUILT:
            all_weno = scheme in (WENO(order=5), FluxFormAdvection(WENO(order=5), WENO(order=5), WENO(order=5)))
            raise NotImplementedError(f"{what}: advection scheme {scheme!r} is not built ({_BUILT_NAME} is: WENO of order 5 in x and y, "
                                      "Centered() in z)" + ("; weno_xyz_tracer_advection_tendency has WENO of order 5 in all three" if all_weno else ""))

    @staticmethod
    def _extra(scheme):
        return ()


def weno_tracer_advection_plan(tracers, u, v, w, G, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    return WenoTracerAdvectionPlan(tracers, u, v, w, G, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos)


def weno_tracer_advection_tendency(tracers, u, v, w, out=None, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    """The advective tendencies G = -div(U c) of the `tracers` (a list of Fields at (Center, Center, Center)) as a list of Fields there: the
    rule of tpg_weno_tracer_advection_tendency (include/tripolar_hip_weno.h) on every interior node -- fifth-order WENO in x and y, centred
    in z, the only `scheme` built.  u at (Face, Center, Center), v at (Center, Face, Center), w at (Center, Center, Face) and the tracers live
    on one TripolarGrid with a halo of at least (3, 3, 1), share element type and device, and the tracers, u and v HAVE THEIR HALOS FILLED;
    w is compute_w_from_continuity's.  `out`: the fields to write into, one per tracer; None allocates CenterField(grid) for each.  More
    than 16 tracers go in several calls.  On an ImmersedBoundaryGrid with `mask_immersed` the nodes under the bottom get 0.  Only the
    interior of each G is written; `fill_halos` then fills those that have conditions.  Returns the list.  Builds a
    WenoTracerAdvectionPlan and runs it once; use weno_tracer_advection_plan in a time loop."""
    tracers = list(tracers)
    out = _tendency_fields(tracers, out, "weno_tracer_advection_tendency")
    plan = WenoTracerAdvectionPlan(tracers, u, v, w, out, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos,
                                   what="weno_tracer_advection_tendency")
    plan()
    return plan.G
