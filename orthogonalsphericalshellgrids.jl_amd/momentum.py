"""The vector-invariant advection tendency of the horizontal velocities on a TripolarGrid: what the AB2 step of the velocities
(time_stepping.py) consumes as Gu, Gv.  The reference's drivers build `HydrostaticFreeSurfaceModel(; momentum_advection = VectorInvariant(),
buoyancy = nothing)` with no Coriolis, no closure and no forcing (examples/bickley_jet.jl:48-55): the whole 3-D tendency of u and v is minus
U.grad(u), minus U.grad(v) in vector-invariant form, and the free-surface gradient is the sub-cycle's.  With it the model step closes on the
device: tendencies -> AB2 -> barotropic mode -> sub-cycle -> correction -> fill -> w -> tendencies.

Everything numeric is tpg_momentum_advection_tendency (include/tripolar_hip_momentum.h, libtripolar_hip_momentum.so): ONE launch for both
fields over the interior nodes i = 1..Nx, j = 1..Ny, k = 1..Nz, in the fields' type T, in exactly this order, with no contraction, every
operation one correctly rounded IEEE operation (kf is a face index, w has Nz + 1 levels):
    Z[i,j,k]  = ((dy_cf[i,j] v[i,j,k] - dy_cf[i-1,j] v[i-1,j,k]) - (dx_fc[i,j] u[i,j,k] - dx_fc[i,j-1] u[i,j-1,k])) / az_ff[i,j]
    P[i,j,k]  = dx_cf[i,j] * v[i,j,k]      Q[i,j,k] = dy_fc[i,j] * u[i,j,k]      A[i,j,kf] = az_cc[i,j] * w[i,j,kf]
    K[i,j,k]  = T(0.5) * (T(0.5) * (u[i,j,k]*u[i,j,k] + u[i+1,j,k]*u[i+1,j,k]) + T(0.5) * (v[i,j,k]*v[i,j,k] + v[i,j+1,k]*v[i,j+1,k]))
 u: zb = T(0.5) * (Z[i,j,k] + Z[i,j+1,k])
    vh = T(0.5) * (T(0.5) * (P[i-1,j,k] + P[i-1,j+1,k]) + T(0.5) * (P[i,j,k] + P[i,j+1,k]))
    hu = -((zb * vh) / dx_fc[i,j])
    bu = (K[i,j,k] - K[i-1,j,k]) / dx_fc[i,j]
    S[i,j,kf] = (T(0.5) * (A[i-1,j,kf] + A[i,j,kf])) * ((u[i,j,kf] - u[i,j,kf-1]) / dz_f[kf])        kf = 1..Nz+1
    vu = (T(0.5) * (S[i,j,k] + S[i,j,k+1])) / az_fc[i,j]
    Gu[i,j,k] = -((hu + vu) + bu)
 v: zb = T(0.5) * (Z[i,j,k] + Z[i+1,j,k])
    uh = T(0.5) * (T(0.5) * (Q[i,j-1,k] + Q[i+1,j-1,k]) + T(0.5) * (Q[i,j,k] + Q[i+1,j,k]))
    hv = (zb * uh) / dy_cf[i,j]
    bv = (K[i,j,k] - K[i,j-1,k]) / dy_cf[i,j]
    R[i,j,kf] = (T(0.5) * (A[i,j-1,kf] + A[i,j,kf])) * ((v[i,j,kf] - v[i,j,kf-1]) / dz_f[kf])
    vv = (T(0.5) * (R[i,j,k] + R[i,j,k+1])) / az_cf[i,j]
    Gv[i,j,k] = -((hv + vv) + bv)
[recalled: Oceananigans' U_dot_∇u / U_dot_∇v for VectorInvariant() with EnstrophyConserving vorticity, the ζ₂wᶠᶜᶠ / ζ₁wᶜᶠᶠ vertical terms and
∂x Khᶜᶜᶜ; parity unpinned, like every operator here].  Leading minus signs are sign flips; a zero divisor divides (the (Face, Center) and
(Face, Face) nodes at the grid poles have zero metrics and give Inf / NaN: a model masks them).  The rule reads u and v one cell beyond the
interior on every side, corner halo cells included (u[Nx+1, 0], v[0, Ny+1]), and w's west column and south row: every halo is at least 1
wide, and the halos of u, v and the horizontal halos of w are the caller's to fill first (the merged fill writes corners; continuity_plan
fills w by default).  Only interior cells of Gu, Gv are written.  On an ImmersedBoundaryGrid the nodes k <= n_fc[i,j] of Gu and
k <= n_cf[i,j] of Gv get 0 inside the same launch -- what mask_immersed_field leaves -- and everything is computed unmasked (Oceananigans'
conditional operators beside an immersed node are out of scope).  The WENO5-upwinded vorticity term of the drivers is a call of its
own, weno_momentum.py; this one keeps refusing every scheme but its own.  The plan form holds its tensors: calling it enqueues on
torch's current stream and allocates nothing (usable inside torch.cuda.graph)."""
from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _ptr
from .boundary_conditions import Center, Face
from .fields import Field
from .reductions import _bare, _grid_table, _metric, z_all_face_spacings
from .time_stepping import _on_device

_LOCS = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}
_SCHEMES = {"enstrophy_conserving": _lib.TPG_MOMENTUM_ENSTROPHY_CONSERVING}
_METRICS = ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff")


def _same(a, b):
    return a is b or a.data is b.data or a.data.data_ptr() == b.data.data_ptr()


class _MomentumTendencyPlan(OperatorPlan):
    """The plan of a vector-invariant momentum tendency, whatever the scheme: the checks of the fields, the metric arrays, ONE C call and the
    halo fill of Gu and Gv.  A scheme's class (MomentumAdvectionPlan here, WenoMomentumAdvectionPlan in weno_momentum.py) supplies what
    differs: `_refuse(scheme, what)`, the smallest halo `_HALO` with the sentence `_HALO_RULE` of its refusal, the band refusal's
    `_BAND_ROWS`, `_LIBRARY` (the names in _lib of the loader and the checker, and the C function) and `_extra(scheme)`, the arguments
    between the mask value and Nx.  `_SPACINGS` names the table of vertical spacings the call takes after the metric planes: dz_f (Nz + 1
    values) unless a class says otherwise."""
    _SPACINGS = ("_z_all_face_spacings", z_all_face_spacings)

    def __init__(self, u, v, w, Gu, Gv, *, scheme, mask_immersed, fill_halos, what):
        self._refuse(scheme, what)
        names = {"u": (u, _LOCS["u"]), "v": (v, _LOCS["v"]), "w": (w, _LOCS["w"]), "Gu": (Gu, _LOCS["u"]), "Gv": (Gv, _LOCS["v"])}
        first = _check_fields(names, what, "u, v, w, Gu and Gv")
        for name, g in (("Gu", Gu), ("Gv", Gv)):
            for other, f in (("u", u), ("v", v), ("w", w)):
                if _same(g, f):
                    raise ValueError(f"{what}: {name} is {other} itself (every node reads its neighbours while they are written)")
        if _same(Gu, Gv):
            raise ValueError(f"{what}: Gu and Gv are one field")
        if any(h < least for h, least in zip((first.Hx, first.Hy, first.Hz), self._HALO)):
            raise ValueError(f"{what}: {self._HALO_RULE} (halo ({first.Hx}, {first.Hy}, {first.Hz}))")
        g = _bare(first.grid)
        if g.global_size and g.Ny != g.global_size[1]:
            raise NotImplementedError(f"{what}: latitude-band grids are not handled: {self._BAND_ROWS}, and the band path of the momentum "
                                      "tendency is not tested yet")
        self.u, self.v, self.w, self.Gu, self.Gv, self.scheme = u, v, w, Gu, Gv, scheme
        dtype, device = u.data.dtype, u.data.device
        load, check, function = self._LIBRARY
        function, check = getattr(getattr(_lib, load)(), function), getattr(_lib, check)
        counts = getattr(first.grid, "column_counts", None) if mask_immersed else None
        nfc, ncf = (None, None) if counts is None else (counts["fc"], counts["cf"])
        with _on_device(device):
            metrics = [_metric(g, name, dtype, device) for name in _METRICS]
            dz = _grid_table(g, *self._SPACINGS, dtype, device)
        held = [u.data, v.data, w.data, Gu.data, Gv.data, *metrics, dz, nfc, ncf]
        args = (*(_ptr(t) for t in held), 0.0, *self._extra(scheme), u.Nx, u.Ny, u.Nz, u.Hx, u.Hy, u.Hz, _lib.ft_of(dtype))
        self._set_call(function, args, check, device, held, (Gu, Gv) if fill_halos else ())


def _tendency_fields(u, out, what):
    """the `out` of a one-shot call: as given, or a new pair of Fields at (Face, Center, Center) and (Center, Face, Center)"""
    if out is not None:
        return out
    if not isinstance(u, Field) or u.loc != _LOCS["u"]:
        raise TypeError(f"{what}: u must be a Field at (Face, Center, Center)")
    return Field(_LOCS["u"], u.grid, name="Gu"), Field(_LOCS["v"], u.grid, name="Gv")


class MomentumAdvectionPlan(_MomentumTendencyPlan):
    """momentum_advection_tendency(u, v, w, out=(Gu, Gv)) with the arguments built once: `plan()` issues ONE
    tpg_momentum_advection_tendency call on torch's current stream and then, with `fill_halos`, ONE HaloFillPlan of Gu and Gv.  It allocates
    nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  On an ImmersedBoundaryGrid with
    `mask_immersed` the (Face, Center) and (Center, Face) count planes and the value 0 go into the call.  The plan holds the tensors of u, v,
    w, Gu and Gv, the metric arrays, the spacings and the count planes: rebuild it if a field's `data` is replaced."""
    _HALO = (1, 1, 1)
    _HALO_RULE = "the rule reads one cell beyond the interior on every side: every halo must be at least 1"
    _BAND_ROWS = "the row Ny + 1 of a band is the exchanged halo row"
    _LIBRARY = ("momentum_lib", "check_momentum", "tpg_momentum_advection_tendency")

    def __init__(self, u, v, w, Gu, Gv, *, scheme="enstrophy_conserving", mask_immersed=True, fill_halos=False, what="momentum_advection_plan"):
        super().__init__(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)

    @staticmethod
    def _refuse(scheme, what):
        if scheme not in _SCHEMES:
            raise NotImplementedError(f"{what}: momentum advection scheme {scheme!r} is not built ('enstrophy_conserving' is; the "
                                      "energy-conserving and WENO vector-invariant schemes are not)")

    @staticmethod
    def _extra(scheme):
        return (_SCHEMES[scheme],)


def momentum_advection_plan(u, v, w, Gu, Gv, *, scheme="enstrophy_conserving", mask_immersed=True, fill_halos=False):
    return MomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos)


def momentum_advection_tendency(u, v, w, out=None, *, scheme="enstrophy_conserving", mask_immersed=True, fill_halos=False):
    """The advective tendencies (Gu, Gv) = (-U.grad(u), -U.grad(v)) in vector-invariant form as Fields at (Face, Center, Center) and
    (Center, Face, Center): the rule of tpg_momentum_advection_tendency on every interior node.  u, v and w at (Center, Center, Face) live
    on one TripolarGrid, share element type and device, and HAVE THEIR HALOS FILLED (corners included; w's horizontal halos too, as
    compute_w_from_continuity leaves them).  `out`: the pair (Gu, Gv) to write into; None allocates XFaceField(grid) and YFaceField(grid).
    On an ImmersedBoundaryGrid with `mask_immersed` the nodes under the bottom get 0.  Only the interiors are written; `fill_halos` then
    fills Gu and Gv.  Returns (Gu, Gv).  Builds a MomentumAdvectionPlan and runs it once; use momentum_advection_plan in a time loop."""
    what = "momentum_advection_tendency"
    Gu, Gv = _tendency_fields(u, out, what)
    plan = MomentumAdvectionPlan(u, v, w, Gu, Gv, scheme=scheme, mask_immersed=mask_immersed, fill_halos=fill_halos, what=what)
    plan()
    return plan.Gu, plan.Gv
