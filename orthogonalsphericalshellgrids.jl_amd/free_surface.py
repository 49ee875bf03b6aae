"""The sub-cycle of a split-explicit free surface on a TripolarGrid: the forward-backward sub-steps of (η, U, V) between the barotropic mode of
the 3-D velocities and their correction (barotropic.py).  The reference's drivers build
HydrostaticFreeSurfaceModel(; grid, free_surface = SplitExplicitFreeSurface(grid; substeps = 30)) (examples/bickley_jet.jl:44-55);
test/runtests.jl:52 uses 12 sub-steps.

Everything numeric is tpg_free_surface_substep (include/tripolar_hip_free_surface.h, libtripolar_hip_free_surface.so): ONE launch per sub-step
over the interior cells, in the fields' type,
    η'[i,j] = η[i,j] - Δτ (((Δyᶠᶜᵃ[i+1,j] U[i+1,j] - Δyᶠᶜᵃ[i,j] U[i,j]) + (Δxᶜᶠᵃ[i,j+1] V[i,j+1] - Δxᶜᶠᵃ[i,j] V[i,j])) / Azᶜᶜᵃ[i,j])
    U'[i,j] = U[i,j] + Δτ (Gᵁ[i,j] - (g Hᶠᶜ) ((η'[i,j] - η'[i-1,j]) / Δxᶠᶜᵃ[i,j]))
    V'[i,j] = V[i,j] + Δτ (Gⱽ[i,j] - (g Hᶜᶠ) ((η'[i,j] - η'[i,j-1]) / Δyᶜᶠᵃ[i,j]))      j ≥ 2;   V'[i,1] = V[i,1]
    η̄ += w η',  Ū += w U',  V̄ += w V'
[recalled: Oceananigans' _split_explicit_free_surface! then _split_explicit_barotropic_velocity! on the new η, ForwardBackwardScheme; parity
unpinned], followed by the halo fill of the three fields just written through the plan machinery of fields.py.  η, U, V ping-pong between
two sets of fields (a sub-step reads its neighbours' cells, so it cannot run in place).  All 2-D fields of a free surface live on
with_halo((Hx, Hy2, Hz), grid), the extended-halo grid (test/runtests.jl:69-71), whose metric planes go into the call.  On an
ImmersedBoundaryGrid the (Face, Center) / (Center, Face) count planes select the column depths H from column_depth_table; nothing is masked.
The plan forms hold their tensors: calling one enqueues on torch's current stream and allocates nothing (usable inside torch.cuda.graph).
Out of scope: AB3 sub-stepping, the free-surface mask, transport-weighted averages, distributed sub-cycling."""
import torch

from . import _lib
from ._operator_plan import OperatorPlan, _check_fields, _ptr, _refuse_window
from .barotropic import column_depth_table
from .boundary_conditions import Center, Face
from .fields import Field, HaloFillPlan
from .grids import is_tripolar, with_halo
from .reductions import _bare, _grid_table

g_Earth = 9.80665                                                  # Oceananigans' default gravitational_acceleration [recalled]

_LOCS = {"eta": (Center, Center, None), "U": (Face, Center, None), "V": (Center, Face, None)}
_STATE = ("eta", "U", "V")


def _loc_of(name):
    return _LOCS["eta" if name.startswith("eta") else name.lstrip("G")[0]]


def _check(fields, what):
    """`fields`: {name: Field} of one sub-step: eta_out, U_out, V_out, eta, U, V, GU, GV and, together or not at all, eta_bar, U_bar, V_bar.
    A z-windowed 3-D field is refused as z-windowed, before its location is looked at; the rest is the shared checker's, then the refusal
    of a distributed grid.  Returns the first field."""
    for f in fields.values():
        if isinstance(f, Field):
            _refuse_window(f, what)
    first = _check_fields({name: (f, _loc_of(name)) for name, f in fields.items()}, what, "the fields of a sub-step",
                          grid_note=" (the free surface's extended-halo grid)")
    if getattr(_bare(first.grid).architecture, "is_distributed", False):
        raise NotImplementedError(f"{what}: distributed sub-cycling is not provided")
    return first


def _column_grid(grid, first, what):
    """the count planes (n_fc, n_cf) of `grid` (None: none) for fields on first.grid"""
    if grid is None:
        return None, None
    if not is_tripolar(grid):
        raise TypeError(f"{what}: grid must be a TripolarGrid or an ImmersedBoundaryGrid of one")
    b = _bare(grid)
    if (b.Nx, b.Ny, b.Nz) != (first.Nx, first.Ny, _bare(first.grid).Nz):
        raise ValueError(f"{what}: grid must share Nx, Ny and Nz with the fields (size {b.Nx}x{b.Ny}x{b.Nz} against "
                         f"{first.Nx}x{first.Ny}x{_bare(first.grid).Nz})")
    counts = getattr(grid, "column_counts", None)
    return (None, None) if counts is None else (counts["fc"], counts["cf"])


class _Substep(OperatorPlan):
    """one tpg_free_surface_substep call with the arguments built once; `weight` None: no averaging"""

    def __init__(self, out, state, G, averages, dtau, g, weight, grid, what):
        names = {"eta_out": out[0], "U_out": out[1], "V_out": out[2], "eta": state[0], "U": state[1], "V": state[2], "GU": G[0], "GV": G[1]}
        if averages is not None:
            names.update({"eta_bar": averages[0], "U_bar": averages[1], "V_bar": averages[2]})
        first = _check(names, what)
        nfc, ncf = _column_grid(grid, first, what)
        ext = _bare(first.grid)
        dtype, device = first.data.dtype, first.data.device
        metrics = [ext.arrays[k] for k in ("dy_fc", "dx_cf", "az_cc", "dx_fc", "dy_cf")]
        if any(m.dtype != dtype or m.device != device for m in metrics):
            raise ValueError(f"{what}: the fields must have the element type and device of their grid's metrics")
        with torch.cuda.device(device):
            depth = _grid_table(ext, "_column_depth_table", column_depth_table, dtype, device)
        held = [f.data for f in names.values()] + metrics + [depth, nfc, ncf]
        bars = [None] * 3 if averages is None else averages
        self._args = (*(_ptr(t) for t in (*out, *state, *G, *bars, *metrics, depth, nfc, ncf)), float(dtau), float(g),
                      0.0 if weight is None else float(weight), first.Nx, first.Ny, ext.Nz, first.Hx, first.Hy, _lib.ft_of(dtype))
        self._set_call(_lib.free_surface_lib().tpg_free_surface_substep, self._args, _lib.check_free_surface, device, held)


def split_explicit_substep(eta_out, U_out, V_out, eta, U, V, GU, GV, dtau, *, gravitational_acceleration=g_Earth, averages=None, weight=1.0,
                           grid=None):
    """ONE call of the rule of tpg_free_surface_substep: (eta, U, V) -> (eta_out, U_out, V_out), all Fields of ONE grid (the free surface's
    extended-halo grid, whose metrics are read) at (Center, Center, Nothing), (Face, Center, Nothing), (Center, Face, Nothing); GU, GV the
    barotropic forcing at U's and V's locations.  The east halo column of U and the north halo row of V are read: the caller has filled them;
    no halo cell is written: the caller's halo fill of the outputs follows.  `averages`: None, or (eta_bar, U_bar, V_bar), which get
    `weight` times the new state added in place.  `grid`: the ImmersedBoundaryGrid whose fc / cf count planes select the column depths
    (None: the full depth everywhere).  Returns (eta_out, U_out, V_out)."""
    if averages is not None and len(averages) != 3:
        raise TypeError("split_explicit_substep: averages are (eta_bar, U_bar, V_bar), given together")
    _Substep((eta_out, U_out, V_out), (eta, U, V), (GU, GV), averages, dtau, gravitational_acceleration, None if averages is None else weight,
             grid, "split_explicit_substep")()
    return eta_out, U_out, V_out


class SplitExplicitFreeSurface:
    """SplitExplicitFreeSurface(grid; substeps, gravitational_acceleration): the 2-D state of a split-explicit free surface.  Owns η, U, V,
    the averages η̄, Ū, V̄ and the forcing Gᵁ, Gⱽ as Fields on `extended_grid` = with_halo((Hx, Hy2, Hz), grid), Hy2 = max(Hy, substeps + 1)
    [recalled: Oceananigans extends the halos of the barotropic fields to substeps + 1; test/runtests.jl:69-71 builds Hy2 = 13 for 12], and
    the ping-pong twins of η, U, V (`twins`).  `grid`: a TripolarGrid or an ImmersedBoundaryGrid of one (its count planes select the column
    depths; the extended grid is built from the underlying one).  `weights`: `substeps` numbers, the averaging weight of each sub-step;
    uniform 1 / substeps by default (Oceananigans' shape function is the caller's to evaluate)."""

    def __init__(self, grid, *, substeps=30, gravitational_acceleration=g_Earth, weights=None):
        what = "SplitExplicitFreeSurface"
        if not is_tripolar(grid):
            raise TypeError(f"{what}: grid must be a TripolarGrid")
        if isinstance(substeps, bool) or not isinstance(substeps, int) or substeps < 1:
            raise ValueError(f"{what}: substeps must be a positive integer, got {substeps!r}")
        weights = [1.0 / substeps] * substeps if weights is None else [float(w) for w in weights]
        if len(weights) != substeps:
            raise ValueError(f"{what}: weights must be {substeps} numbers, one per sub-step (got {len(weights)})")
        base = _bare(grid)
        if getattr(base.architecture, "is_distributed", False):
            raise NotImplementedError(f"{what}: distributed sub-cycling is not provided")
        self.grid, self.substeps, self.gravitational_acceleration, self.weights = grid, substeps, float(gravitational_acceleration), weights
        Hy2 = max(base.Hy, substeps + 1)
        self.extended_grid = ext = base if Hy2 == base.Hy else with_halo((base.Hx, Hy2, base.Hz), base)
        new = lambda name, key: Field(_LOCS[key], ext, name=name)
        self.eta, self.U, self.V = new("η", "eta"), new("U", "U"), new("V", "V")
        self.eta_bar, self.U_bar, self.V_bar = new("η̄", "eta"), new("Ū", "U"), new("V̄", "V")
        self.GU, self.GV = new("Gᵁ", "U"), new("Gⱽ", "V")
        self.twins = (new("η twin", "eta"), new("U twin", "U"), new("V twin", "V"))

    @property
    def state(self):
        return self.eta, self.U, self.V

    @property
    def averages(self):
        return self.eta_bar, self.U_bar, self.V_bar

    def __repr__(self):
        return (f"SplitExplicitFreeSurface(substeps={self.substeps}, gravitational_acceleration={self.gravitational_acceleration}) on "
                f"{self.extended_grid!r}")


def subcycle_schedule(substeps):
    """(copy_first, [(src, dst)] * substeps): which of the two field sets (0: the caller's η, U, V; 1: the twins) each sub-step reads and
    writes so that the LAST one writes set 0.  The sets alternate; with an odd count the first sub-step has to read the twins, which then
    get a copy of the state first (`copy_first`)."""
    steps = [((substeps - s + 1) % 2, (substeps - s) % 2) for s in range(1, substeps + 1)]
    return steps[0][0] == 1, steps


class SplitExplicitSubcyclePlan:
    """The whole sub-cycle with the arguments built once: `plan()` issues on torch's current stream, `substeps` times, ONE
    tpg_free_surface_substep call and ONE HaloFillPlan of the three fields it wrote, alternating between the free surface's η, U, V and their
    twins so that the final state is in η, U, V for odd and even `substeps` (odd: the twins first get a device copy of the state).  With
    `average` the averages are zeroed first, every sub-step adds weights[s] times its new state to them, and their halos are filled once at
    the end.  It allocates nothing when called and is a single chain of launches, so it replays inside torch.cuda.graph.  The halos of η, U,
    V must be filled on entry (the first sub-step reads U's east column and V's north row).  On an ImmersedBoundaryGrid the fc / cf count
    planes and column_depth_table go into every call.  The plan holds the tensors of the fields: rebuild it if a field's `data` is replaced."""

    def __init__(self, free_surface, dtau, *, average=True, what="split_explicit_subcycle_plan"):
        fs = free_surface
        if not isinstance(fs, SplitExplicitFreeSurface):
            raise TypeError(f"{what}: free_surface must be a SplitExplicitFreeSurface")
        self.free_surface, self.dtau = fs, float(dtau)
        sets = (fs.state, fs.twins)
        averages = fs.averages if average else None
        self._copy_first, self.schedule = subcycle_schedule(fs.substeps)
        self._steps = [_Substep(sets[dst], sets[src], (fs.GU, fs.GV), averages, dtau, fs.gravitational_acceleration,
                                fs.weights[s] if average else None, fs.grid, what) for s, (src, dst) in enumerate(self.schedule)]
        self._fills = [HaloFillPlan(list(fields)) for fields in sets]
        self._averages = averages
        self._fill_averages = HaloFillPlan(list(averages)) if average else None

    def __call__(self):
        fs = self.free_surface
        if self._averages is not None:
            for f in self._averages:
                f.data.zero_()
        if self._copy_first:
            for f, t in zip(fs.state, fs.twins):
                t.data.copy_(f.data)
        for step, (_, dst) in zip(self._steps, self.schedule):
            step()
            self._fills[dst]()
        if self._fill_averages is not None:
            self._fill_averages()
        return self


def split_explicit_subcycle_plan(free_surface, dtau, *, average=True):
    return SplitExplicitSubcyclePlan(free_surface, dtau, average=average)
