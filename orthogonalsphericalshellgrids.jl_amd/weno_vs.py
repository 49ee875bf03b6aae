"""The vector-invariant advection tendency of the horizontal velocities of the drivers' scheme: examples/bickley_jet.jl:49 and
examples/distributed_bickley_jet.jl:51 have `momentum_advection = WENOVectorInvariant(vorticity_order = 5)`, which is Oceananigans'
    VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = VelocityStencil(), vertical_scheme = WENO(order = 5),
                    kinetic_energy_gradient_scheme = WENO(order = 5), divergence_scheme = WENO(order = 5),
                    upwinding = OnlySelfUpwinding(cross_scheme = WENO(order = 5)))
-- weno_vi.py's scheme with the smoothness of the WENO5 vorticity reconstruction measured on the velocities (VelocityStencil) instead of
on the vorticity itself (DefaultStencil).  The record is weno_vs.BUILT.  The result is the Gu, Gv of the AB2 step of the velocities.

Everything numeric is tpg_weno_vs_momentum_advection_tendency (libtripolar_hip_weno_vs.so).  THE RULE is written out once, in
include/tripolar_hip_weno_vs.h: include/tripolar_hip_weno_vi.h's with zr inside hu and hv replaced by W5V, whose smoothness indicators are
the halved sums of the indicators of UB = u averaged in y and VB = v averaged in x onto (Face, Face) [recalled: Oceananigans' biased WENO
weights for VelocityStencil -- the smoothness indicators of the tangential stencils of the two averaged velocities, summed and halved
(beta_sum); parity unpinned, like every operator here].  The rule reads no cell weno_vi's does not read: the halo is at least (3, 3, 1),
the halos of u, v and the horizontal halos of w are the caller's to fill first, only interior cells of Gu, Gv are written, the vertical
spacings are z_center_spacings (dz_c), and on an ImmersedBoundaryGrid the nodes k <= n_fc[i,j] of Gu and k <= n_cf[i,j] of Gv get 0 inside
the call.

Stays out: the constructor osg.WENOVectorInvariant() keeps raising (its message is pinned by older tests and now out of
date: this module builds what it says is missing); other orders; the centred vertical term with this stencil; latitude bands; the Julia
hooks.

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
import dataclasses

from . import weno_vi
from .momentum import _MomentumTendencyPlan, _tendency_fields
from .reductions import z_center_spacings
from .weno import WENO
from .weno_momentum import DefaultStencil, EnstrophyConserving, VectorInvariant, VelocityStencil

BUILT = dataclasses.replace(weno_vi.BUILT, vorticity_stencil=VelocityStencil())
_BUILT_NAME = ("VectorInvariant(vorticity_scheme=WENO(order=5), vorticity_stencil=VelocityStencil(), vertical_scheme=WENO(order=5), "
               "kinetic_energy_gradient_scheme=WENO(order=5), divergence_scheme=WENO(order=5), "
               "upwinding=OnlySelfUpwinding(cross_scheme=WENO(order=5)))")


def _refuse(scheme, what):
    if isinstance(scheme, VectorInvariant):
        if isinstance(scheme.vorticity_scheme, EnstrophyConserving) or scheme == VectorInvariant():
            raise NotImplementedError(f"{what}: the enstrophy-conserving vorticity term is momentum_advection_plan's "
                                      f"(scheme='enstrophy_conserving'); this call builds {_BUILT_NAME}")
        orders = [s.order for s in (scheme.vorticity_scheme, scheme.vertical_scheme, scheme.kinetic_energy_gradient_scheme,
                                    scheme.divergence_scheme, getattr(scheme.upwinding, "cross_scheme", None)) if isinstance(s, WENO)]
        if any(order != 5 for order in orders):
            raise NotImplementedError(f"{what}: WENO of order {next(o for o in orders if o != 5)} is not built ({_BUILT_NAME} is: order 5 only)")
        if isinstance(scheme.vorticity_stencil, DefaultStencil):
            raise NotImplementedError(f"{what}: DefaultStencil smoothness is weno_vi_momentum_advection_plan's (weno_vi.BUILT; with the centred "
                                      f"vertical term and kinetic-energy gradient, weno_momentum_advection_plan's); this call builds {_BUILT_NAME}")
    if not isinstance(scheme, VectorInvariant) or scheme != BUILT:
        raise NotImplementedError(f"{what}: momentum advection scheme {scheme!r} is not built ({_BUILT_NAME} is)")


class WenoVsMomentumAdvectionPlan(_MomentumTendencyPlan):
    """weno_vs_momentum_advection_tendency(u, v, w, out=(Gu, Gv)) with the arguments built once: `plan()` issues ONE
    tpg_weno_vs_momentum_advection_tendency call on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of Gu and Gv.  It
    allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  On an ImmersedBoundaryGrid
    with `mask_immersed` the (Face, Center) and (Center, Face) count planes and the value 0 go into the call.  The plan holds the tensors of
    u, v, w, Gu and Gv, the metric arrays, the spacings and the count planes: rebuild it if a field's `data` is replaced."""
    _HALO = (3, 3, 1)
    _HALO_RULE = weno_vi.WenoViMomentumAdvectionPlan._HALO_RULE    # the rule reads no cell weno_vi's does not read
    _BAND_ROWS = weno_vi.WenoViMomentumAdvectionPlan._BAND_ROWS
    _LIBRARY = ("weno_vs_lib", "check_weno_vs", "tpg_weno_vs_momentum_advection_tendency")
    _SPACINGS = ("_z_center_spacings", z_center_spacings)          # dz_c, Nz values: the flux-form vertical term has no dz_f
    _refuse = staticmethod(_refuse)

    def __init__(self, u, v, w, Gu, Gv, *, scheme=BUILT, mask_immersed=True, fill_halos=False, what="weno_vs_momentum_advection_plan"):
        super().__init__(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)

    @staticmethod
    def _extra(scheme):
        return ()


def weno_vs_momentum_advection_plan(u, v, w, Gu, Gv, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    return WenoVsMomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos)


def weno_vs_momentum_advection_tendency(u, v, w, out=None, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    """The advective tendencies (Gu, Gv) = (-U.grad(u), -U.grad(v)) of the drivers' WENOVectorInvariant(vorticity_order = 5), as Fields at
    (Face, Center, Center) and (Center, Face, Center): the rule of tpg_weno_vs_momentum_advection_tendency
    (include/tripolar_hip_weno_vs.h) on every interior node, the only `scheme` built (weno_vs.BUILT).  The arguments are
    weno_vi_momentum_advection_tendency's: u, v and w live on one TripolarGrid with a halo of at least (3, 3, 1), share element type and
    device, and HAVE THEIR HALOS FILLED (corners included; w's horizontal halos too).  `out`: the pair (Gu, Gv) to write into; None
    allocates XFaceField(grid) and YFaceField(grid).  On an ImmersedBoundaryGrid with `mask_immersed` the nodes under the bottom get 0.
    Only the interiors are written; `fill_halos` then fills Gu and Gv.  Returns (Gu, Gv).  Builds a WenoVsMomentumAdvectionPlan and runs it
    once; use weno_vs_momentum_advection_plan in a time loop."""
    what = "weno_vs_momentum_advection_tendency"
    _refuse(scheme, what)
    Gu, Gv = _tendency_fields(u, out, what)
    plan = WenoVsMomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)
    plan()
    return plan.Gu, plan.Gv
