#!/usr/bin/env python3
"""examples/hydrostatic_model_step.py with the closure every realistic model carries:
`closure = VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν = 1e-2, κ = 1e-4)`.  Right after each AB2 update the implicit
step solves (1 - Δt ∂z κ ∂z) ϕ = f in every column, in place (Oceananigans' implicit_step!):

  the tendencies          as in hydrostatic_model_step.py;
  the AB2 steps           b, then u and v with the barotropic forcing -- their halo fills move behind the implicit step;
  the implicit step       u with ν and the (Face, Center) counts, v with ν and the (Center, Face) counts, b with κ and the (Center, Center)
                          counts: THREE launches (implicit_step_plan), then ONE halo fill per call;
  the rest                the barotropic mode, the sub-cycle, the correction and w.

The same grid, bottom, jet and stratification.  Nine plans built once.  The step runs eagerly from a saved start, then the same chain is
captured into ONE graph and replayed from the same start: the script prints that the two agree bit for bit.
Run on an MI355X:  python examples/vertical_diffusion_model_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg
from bickley_model_step import DEPTH, DT, HALO, POLE_LAT, POLE_LON, SIZE, STEPS, SUBSTEPS, bottom_height, same_bits, u_initial, v_initial
from hydrostatic_model_step import b_initial

NU, KAPPA = 1e-2, 1e-4                                             # m2/s


def main():
    torch.cuda.set_device(0)
    underlying = osg.TripolarGrid(size=SIZE, halo=HALO, z=(-DEPTH, 0), first_pole_longitude=POLE_LON, north_poles_latitude=POLE_LAT)
    for name in ("dx_fc", "dy_fc", "az_fc", "az_ff", "dy_cf"):    # zero metrics at the two grid poles, where the rules divide by them: land here
        metric = underlying.arrays[name]
        metric[metric == 0] = 1.0
    grid = osg.ImmersedBoundaryGrid(underlying, osg.GridFittedBottom(bottom_height))
    fs = osg.SplitExplicitFreeSurface(grid, substeps=SUBSTEPS)
    for name in ("dx_fc", "dy_fc"):
        metric = fs.extended_grid.arrays[name]
        metric[metric == 0] = 1.0
    u, v, w, b, p = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.CenterField(grid), osg.CenterField(grid)
    Gu, Gv, Gu_prev, Gv_prev = osg.XFaceField(grid), osg.YFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid)
    Gb, Gb_prev = osg.CenterField(grid), osg.CenterField(grid)
    Ubar, Vbar = osg.Field(fs.U.loc, fs.extended_grid), osg.Field(fs.V.loc, fs.extended_grid)
    u.set_(u_initial)
    v.set_(v_initial)
    b.set_(b_initial)
    osg.mask_immersed_field([u, v, b], 0)
    osg.fill_halo_regions([u, v, b, fs.eta])
    continuity = osg.continuity_plan(u, v, w)
    continuity()
    coriolis = osg.HydrostaticSphericalCoriolis()
    closure = osg.VerticalScalarDiffusivity(osg.VerticallyImplicitTimeDiscretization(), nu=NU, kappa={"b": KAPPA})
    tracer_tendency = osg.weno_tracer_advection_plan([b], u, v, w, [Gb])
    momentum_tendency = osg.momentum_advection_plan(u, v, w, Gu, Gv)
    hydrostatic = osg.hydrostatic_tendencies_plan(u, v, Gu, Gv, coriolis=coriolis, b=b, pressure=p)     # accumulates: after the advection plan
    ab2_tracer = osg.ab2_step_plan([b], [Gb], [Gb_prev], DT)
    ab2 = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gu_prev, Gv_prev, DT, GU=fs.GU, GV=fs.GV)
    implicit = osg.implicit_step_plan(u, v, {"b": b}, closure, DT, fill_halos=True)                        # the fills the AB2 plans had
    mode = osg.barotropic_mode_plan(u, v, Ubar, Vbar)
    subcycle = osg.split_explicit_subcycle_plan(fs, DT / SUBSTEPS)
    correction = osg.barotropic_correction_plan(u, v, fs.U, fs.V, Ubar, Vbar)
    momentum_tendency()
    hydrostatic()
    tracer_tendency()
    for prev, now in ((Gu_prev, Gu), (Gv_prev, Gv), (Gb_prev, Gb)):
        prev.data.copy_(now.data)

    def step():
        tracer_tendency()
        momentum_tendency()
        hydrostatic()
        ab2_tracer()
        ab2()
        implicit()
        mode()
        fs.U.data.copy_(Ubar.data)
        fs.V.data.copy_(Vbar.data)
        subcycle()
        correction()
        continuity()

    def report(tag):
        inner = lambda f: f.interior()[..., :-1, :]                # row Ny apart: its east half is the fold's                # noqa: E731
        peak = lambda f: inner(f)[torch.isfinite(inner(f))].abs().max().item()                                                 # noqa: E731
        print(f"{tag}: max|u| {peak(u):.4f}, max|v| {peak(v):.4f}, max|w| {peak(w):.3e} m/s, max|Gu| {peak(Gu):.3e} m/s2, "
              f"max|p| {peak(p):.4f} m2/s2, max|η| {peak(fs.eta):.4f} m, b in [{inner(b).min().item():.5f}, {inner(b).max().item():.5f}]")

    state = [u, v, w, b, p, Gu, Gv, Gb, Gu_prev, Gv_prev, Gb_prev, Ubar, Vbar, fs.GU, fs.GV, *fs.state, *fs.twins, *fs.averages]
    start = [f.data.clone() for f in state]
    for n in range(STEPS):
        step()
        report(f"step {n}")
    torch.cuda.synchronize()
    eager = [f.data.clone() for f in state]
    graph = torch.cuda.CUDAGraph()                                 # the same chain as ONE graph: nothing in it allocates
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    for f, t in zip(state, start):
        f.data.copy_(t)
    for n in range(STEPS):
        graph.replay()
        report(f"step {n} (graph)")
    torch.cuda.synchronize()
    agree = all(same_bits(f.data, t) for f, t in zip(state, eager))
    print(f"eager and replayed graph agree bit for bit on all {len(state)} fields: {agree}")
    assert agree


if __name__ == "__main__":
    main()
