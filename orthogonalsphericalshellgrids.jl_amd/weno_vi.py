"""The vector-invariant advection tendency of the horizontal velocities with upwinding in every term: the WENO5-upwinded vorticity flux of
weno_momentum.py, the upwinded vertical term -- the horizontal divergence upwinded against the advected velocity itself, the flux of u and
v in z reconstructed by WENO -- and the upwinded kinetic-energy gradient.  examples/bickley_jet.jl:49 and
examples/distributed_bickley_jet.jl:51 have `momentum_advection = WENOVectorInvariant(vorticity_order = 5)`; what is built here is
Oceananigans'
    VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(), vertical_scheme = WENO(order = 5),
                    kinetic_energy_gradient_scheme = WENO(order = 5), divergence_scheme = WENO(order = 5),
                    upwinding = OnlySelfUpwinding(cross_scheme = WENO(order = 5)))
which the smoothness stencil of the vorticity reconstruction alone separates from the drivers' scheme (DefaultStencil here, VelocityStencil
there: WENOVectorInvariant() keeps raising).  The result is the Gu, Gv of the AB2 step of the velocities.

Everything numeric is tpg_weno_vi_momentum_advection_tendency (libtripolar_hip_weno_vi.so).  THE RULE is written out once, in
include/tripolar_hip_weno_vi.h -- in the fields' type T, in exactly that order, with no contraction, every operation one correctly rounded
IEEE operation [recalled: Oceananigans' upwinded divergence flux and Bernoulli head for VectorInvariant with WENO schemes and
OnlySelfUpwinding, FunctionStencil smoothness, the cross terms as the symmetric fourth-order value; parity unpinned, like every operator
here].  The rule reads u and v three cells beyond the interior in x and y (corner halo cells included), w two cells, and in z the planes
0 and Nz + 1 only (the faces beside a wall drop their order): the halo is at least (3, 3, 1), and the halos of u, v and the horizontal halos
of w are the caller's to fill first -- the rows Ny+1..Ny+3 are the Zipper's.  Only interior cells of Gu, Gv are written.  The vertical
spacings are z_center_spacings (dz_c); there is no dz_f in this call.  On an ImmersedBoundaryGrid the nodes k <= n_fc[i,j] of Gu and
k <= n_cf[i,j] of Gv get 0 inside the call, and everything is computed unmasked.

Stays out: VelocityStencil smoothness (weno_vs.py builds it, as a call of its own), other orders, Oceananigans' drop of the order beside the south wall and immersed nodes,
latitude bands, the Julia hooks.

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
from .momentum import _MomentumTendencyPlan, _tendency_fields
from .reductions import z_center_spacings
from .weno import WENO
from .weno_momentum import DefaultStencil, EnstrophyConserving, OnlySelfUpwinding, VectorInvariant, VelocityStencil  # noqa: F401

BUILT = VectorInvariant(vorticity_scheme=WENO(order=5), vorticity_stencil=DefaultStencil(), vertical_scheme=WENO(order=5),
                        kinetic_energy_gradient_scheme=WENO(order=5), divergence_scheme=WENO(order=5),
                        upwinding=OnlySelfUpwinding(cross_scheme=WENO(order=5)))
_BUILT_NAME = ("VectorInvariant(vorticity_scheme=WENO(order=5), vorticity_stencil=DefaultStencil(), vertical_scheme=WENO(order=5), "
               "kinetic_energy_gradient_scheme=WENO(order=5), divergence_scheme=WENO(order=5), "
               "upwinding=OnlySelfUpwinding(cross_scheme=WENO(order=5)))")


def _refuse(scheme, what):
    if isinstance(scheme, VectorInvariant):
        if isinstance(scheme.vorticity_scheme, EnstrophyConserving) or scheme == VectorInvariant():
            raise NotImplementedError(f"{what}: the enstrophy-conserving vorticity term is momentum_advection_plan's "
                                      f"(scheme='enstrophy_conserving'); this call builds {_BUILT_NAME}")
        if isinstance(scheme.vorticity_stencil, VelocityStencil):
            raise NotImplementedError(f"{what}: VelocityStencil smoothness is not built ({_BUILT_NAME} is: DefaultStencil only)")
        orders = [s.order for s in (scheme.vorticity_scheme, scheme.vertical_scheme, scheme.kinetic_energy_gradient_scheme,
                                    scheme.divergence_scheme, getattr(scheme.upwinding, "cross_scheme", None)) if isinstance(s, WENO)]
        if any(order != 5 for order in orders):
            raise NotImplementedError(f"{what}: WENO of order {next(o for o in orders if o != 5)} is not built ({_BUILT_NAME} is: order 5 only)")
        if scheme.kinetic_energy_gradient_scheme is None and scheme.divergence_scheme is None and scheme.upwinding is None:
            raise NotImplementedError(f"{what}: momentum advection scheme {scheme!r} is not built here: the centred vertical term and "
                                      f"kinetic-energy gradient are weno_momentum_advection_plan's; this call builds {_BUILT_NAME}")
    if not isinstance(scheme, VectorInvariant) or scheme != BUILT:
        raise NotImplementedError(f"{what}: momentum advection scheme {scheme!r} is not built ({_BUILT_NAME} is)")


class WenoViMomentumAdvectionPlan(_MomentumTendencyPlan):
    """weno_vi_momentum_advection_tendency(u, v, w, out=(Gu, Gv)) with the arguments built once: `plan()` issues ONE
    tpg_weno_vi_momentum_advection_tendency call on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of Gu and Gv.  It
    allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  On an ImmersedBoundaryGrid
    with `mask_immersed` the (Face, Center) and (Center, Face) count planes and the value 0 go into the call.  The plan holds the tensors of
    u, v, w, Gu and Gv, the metric arrays, the spacings and the count planes: rebuild it if a field's `data` is replaced."""
    _HALO = (3, 3, 1)
    _HALO_RULE = ("the rule reads three cells beyond the interior in x and y and, in z, the planes 0 and Nz + 1 only (the faces beside a wall "
                  "drop their order): the halo must be at least (3, 3, 1)")
    _BAND_ROWS = "the rows Ny + 1 .. Ny + 3 of a band are exchanged halo rows"
    _LIBRARY = ("weno_vi_lib", "check_weno_vi", "tpg_weno_vi_momentum_advection_tendency")
    _SPACINGS = ("_z_center_spacings", z_center_spacings)          # dz_c, Nz values: the flux-form vertical term has no dz_f
    _refuse = staticmethod(_refuse)

    def __init__(self, u, v, w, Gu, Gv, *, scheme=BUILT, mask_immersed=True, fill_halos=False, what="weno_vi_momentum_advection_plan"):
        super().__init__(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)

    @staticmethod
    def _extra(scheme):
        return ()


def weno_vi_momentum_advection_plan(u, v, w, Gu, Gv, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    return WenoViMomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos)


def weno_vi_momentum_advection_tendency(u, v, w, out=None, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    """The advective tendencies (Gu, Gv) = (-U.grad(u), -U.grad(v)) in vector-invariant form with upwinding in every term, as Fields at
    (Face, Center, Center) and (Center, Face, Center): the rule of tpg_weno_vi_momentum_advection_tendency
    (include/tripolar_hip_weno_vi.h) on every interior node, the only `scheme` built (weno_vi.BUILT).  u, v and w at
    (Center, Center, Face) live on one TripolarGrid with a halo of at least (3, 3, 1), share element type and device, and HAVE THEIR HALOS
    FILLED (corners included; w's horizontal halos too, as compute_w_from_continuity leaves them).  `out`: the pair (Gu, Gv) to write into;
    None allocates XFaceField(grid) and YFaceField(grid).  On an ImmersedBoundaryGrid with `mask_immersed` the nodes under the bottom get
    0.  Only the interiors are written; `fill_halos` then fills Gu and Gv.  Returns (Gu, Gv).  Builds a WenoViMomentumAdvectionPlan and
    runs it once; use weno_vi_momentum_advection_plan in a time loop."""
    what = "weno_vi_momentum_advection_tendency"
    _refuse(scheme, what)
    Gu, Gv = _tendency_fields(u, out, what)
    plan = WenoViMomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)
    plan()
    return plan.Gu, plan.Gv
