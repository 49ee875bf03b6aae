"""The vector-invariant advection tendency of the horizontal velocities with the WENO5-upwinded vorticity term: the momentum half of the
scheme the reference's drivers build.  examples/bickley_jet.jl:49 and examples/distributed_bickley_jet.jl:51 have
`momentum_advection = WENOVectorInvariant(vorticity_order = 5)`; what is built here is its vorticity term, Oceananigans'
`VectorInvariant(vorticity_scheme = WENO(order = 5), vorticity_stencil = DefaultStencil(), vertical_scheme = EnergyConserving())`: the
vertical vorticity reconstructed with fifth-order WENO against the transverse velocity, the vertical term and the kinetic-energy gradient
those of momentum_advection_tendency (momentum.py, the enstrophy-conserving and centred vorticity term).  The result is the Gu, Gv of the AB2
step of the velocities, as that call's is.

Everything numeric is tpg_weno_momentum_advection_tendency (libtripolar_hip_weno_momentum.so).  THE RULE is written out once, in
include/tripolar_hip_weno_momentum.h: everything is tpg_momentum_advection_tendency's but
    hu = -(vhat * zr),  vhat = vh / dx_fc[i,j],  zr = vhat >= 0 ? W5(Z[i, j-2 .. j+2]) : W5(Z[i, j+3 .. j-1])
    hv =   uhat * zr,   uhat = uh / dy_cf[i,j],  zr = uhat >= 0 ? W5(Z[i-2 .. i+2, j]) : W5(Z[i+3 .. i-1, j])
with W5 the face value R of include/tripolar_hip_weno.h -- in the fields' type T, in exactly that order, with no contraction, every
operation one correctly rounded IEEE operation [recalled: Oceananigans' VectorInvariant with a WENO vorticity scheme and DefaultStencil
smoothness; parity unpinned, like every operator here].  The rule reads u and v three cells beyond the interior in x and y (two crosses,
corner halo cells included) and one in z: the halo is at least (3, 3, 1), and the halos of u, v and the horizontal halos of w are the
caller's to fill first -- the rows Ny+1..Ny+3 are the Zipper's.  Only interior cells of Gu, Gv are written.  A non-finite Z (zero az_ff at
a pole) reaches every node whose window holds it: a model masks them.  On an ImmersedBoundaryGrid the nodes k <= n_fc[i,j] of Gu and
k <= n_cf[i,j] of Gv get 0 inside the same launch, and everything is computed unmasked.

Stays out here: the upwinded divergence flux, the upwinded kinetic-energy gradient and WENO in z of WENOVectorInvariant, which are a call
of their own (weno_vi.py).  Stays out everywhere: VelocityStencil smoothness, other orders, Oceananigans' drop of the order beside the south wall and immersed nodes, latitude
bands, the Julia hooks.

The plan form holds its tensors: calling it enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
from dataclasses import dataclass

from .momentum import _MomentumTendencyPlan, _tendency_fields
from .weno import WENO, Centered


@dataclass(frozen=True)
class EnergyConserving:
    """Oceananigans' `EnergyConserving()`: a plain record (as a vertical scheme: the zeta2 w / zeta1 w terms of momentum.py)"""


@dataclass(frozen=True)
class EnstrophyConserving:
    """Oceananigans' `EnstrophyConserving()`: a plain record (as a vorticity scheme: what momentum_advection_plan builds)"""


@dataclass(frozen=True)
class DefaultStencil:
    """Oceananigans' `DefaultStencil()`: the smoothness indicators of the vorticity reconstruction are formed from the vorticity itself"""


@dataclass(frozen=True)
class VelocityStencil:
    """Oceananigans' `VelocityStencil()`: smoothness indicators formed from the velocities.  A record only: not built."""


@dataclass(frozen=True)
class OnlySelfUpwinding:
    """Oceananigans' `OnlySelfUpwinding(; cross_scheme)`: in the divergence flux and the kinetic-energy gradient only the term in the
    advected velocity's own direction is upwinded; the cross term is the symmetric value of `cross_scheme`.  A plain record."""
    cross_scheme: object = Centered()


@dataclass(frozen=True)
class VectorInvariant:
    """Oceananigans' `VectorInvariant(; vorticity_scheme, vertical_scheme, vorticity_stencil, kinetic_energy_gradient_scheme,
    divergence_scheme, upwinding)`: a plain record.  VectorInvariant() is the default, the enstrophy-conserving vorticity term of
    momentum_advection_plan.  The last three are None where nothing is upwinded beside the vorticity: the centred, energy-conserving
    vertical term and kinetic-energy gradient."""
    vorticity_scheme: object = EnstrophyConserving()
    vertical_scheme: object = EnergyConserving()
    vorticity_stencil: object = DefaultStencil()
    kinetic_energy_gradient_scheme: object = None
    divergence_scheme: object = None
    upwinding: object = None


BUILT = VectorInvariant(vorticity_scheme=WENO(order=5), vertical_scheme=EnergyConserving(), vorticity_stencil=DefaultStencil())
_BUILT_NAME = "VectorInvariant(vorticity_scheme=WENO(order=5), vertical_scheme=EnergyConserving(), vorticity_stencil=DefaultStencil())"


def WENOVectorInvariant(vorticity_order=5):
    """The reference drivers' `WENOVectorInvariant(vorticity_order = 5)`.  Not built: always raises, naming what is."""
    raise NotImplementedError(
        f"WENOVectorInvariant(vorticity_order={vorticity_order!r}) is not built: beside the WENO vorticity term it has the upwinded divergence "
        f"flux, the upwinded kinetic-energy gradient and VelocityStencil smoothness.  The first two are built with DefaultStencil smoothness as "
        f"weno_vi.BUILT (weno_vi_momentum_advection_plan); VelocityStencil smoothness is missing.  Its vorticity term alone is "
        f"built as {_BUILT_NAME}: pass that (weno_momentum.BUILT, the default)")


def _refuse(scheme, what):
    if isinstance(scheme, VectorInvariant):
        if isinstance(scheme.vorticity_scheme, EnstrophyConserving) or scheme == VectorInvariant():
            raise NotImplementedError(f"{what}: the enstrophy-conserving vorticity term is momentum_advection_plan's "
                                      f"(scheme='enstrophy_conserving'); this call builds {_BUILT_NAME}")
        if isinstance(scheme.vorticity_scheme, WENO) and scheme.vorticity_scheme.order != 5:
            raise NotImplementedError(f"{what}: WENO of order {scheme.vorticity_scheme.order} is not built ({_BUILT_NAME} is: order 5 only)")
        if isinstance(scheme.vorticity_stencil, VelocityStencil):
            raise NotImplementedError(f"{what}: VelocityStencil smoothness is not built ({_BUILT_NAME} is: DefaultStencil only)")
        if any(x is not None for x in (scheme.kinetic_energy_gradient_scheme, scheme.divergence_scheme, scheme.upwinding)):
            raise NotImplementedError(f"{what}: momentum advection scheme {scheme!r} is not built here: the upwinded divergence flux and "
                                      f"kinetic-energy gradient are weno_vi_momentum_advection_plan's; this call builds {_BUILT_NAME}")
    if not isinstance(scheme, VectorInvariant) or scheme != BUILT:
        raise NotImplementedError(f"{what}: momentum advection scheme {scheme!r} is not built ({_BUILT_NAME} is)")


class WenoMomentumAdvectionPlan(_MomentumTendencyPlan):
    """weno_momentum_advection_tendency(u, v, w, out=(Gu, Gv)) with the arguments built once: `plan()` issues ONE
    tpg_weno_momentum_advection_tendency call on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of Gu and Gv.  It
    allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  On an ImmersedBoundaryGrid
    with `mask_immersed` the (Face, Center) and (Center, Face) count planes and the value 0 go into the call.  The plan holds the tensors of
    u, v, w, Gu and Gv, the metric arrays, the spacings and the count planes: rebuild it if a field's `data` is replaced."""
    _HALO = (3, 3, 1)
    _HALO_RULE = "the rule reads three cells beyond the interior in x and y and one in z: the halo must be at least (3, 3, 1)"
    _BAND_ROWS = "the rows Ny + 1 .. Ny + 3 of a band are exchanged halo rows"
    _LIBRARY = ("weno_momentum_lib", "check_weno_momentum", "tpg_weno_momentum_advection_tendency")
    _refuse = staticmethod(_refuse)

    def __init__(self, u, v, w, Gu, Gv, *, scheme=BUILT, mask_immersed=True, fill_halos=False, what="weno_momentum_advection_plan"):
        super().__init__(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)

    @staticmethod
    def _extra(scheme):
        return ()


def weno_momentum_advection_plan(u, v, w, Gu, Gv, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    return WenoMomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos)


def weno_momentum_advection_tendency(u, v, w, out=None, *, scheme=BUILT, mask_immersed=True, fill_halos=False):
    """The advective tendencies (Gu, Gv) = (-U.grad(u), -U.grad(v)) in vector-invariant form with the WENO5-upwinded vorticity term, as
    Fields at (Face, Center, Center) and (Center, Face, Center): the rule of tpg_weno_momentum_advection_tendency
    (include/tripolar_hip_weno_momentum.h) on every interior node, the only `scheme` built.  u, v and w at (Center, Center, Face) live on one
    TripolarGrid with a halo of at least (3, 3, 1), share element type and device, and HAVE THEIR HALOS FILLED (corners included; w's
    horizontal halos too, as compute_w_from_continuity leaves them).  `out`: the pair (Gu, Gv) to write into; None allocates
    XFaceField(grid) and YFaceField(grid).  On an ImmersedBoundaryGrid with `mask_immersed` the nodes under the bottom get 0.  Only the
    interiors are written; `fill_halos` then fills Gu and Gv.  Returns (Gu, Gv).  Builds a WenoMomentumAdvectionPlan and runs it once; use
    weno_momentum_advection_plan in a time loop."""
    what = "weno_momentum_advection_tendency"
    _refuse(scheme, what)
    Gu, Gv = _tendency_fields(u, out, what)
    plan = WenoMomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)
    plan()
    return plan.Gu, plan.Gv
