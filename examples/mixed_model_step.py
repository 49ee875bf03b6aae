#!/usr/bin/env python3
"""examples/forced_model_step.py with an ocean that reacts to what is done to it: the surface is COOLED, and the unstable column that
cooling produces is mixed by convective adjustment,

  `ConvectiveAdjustmentVerticalDiffusivity(convective_κz = 0.1, convective_νz = 0.1, background_κz = 1e-4, background_νz = 1e-2)`,

in place of the constant ν and κ of `VerticalScalarDiffusivity`.  The implicit step gains ONE launch (mixed_implicit_step_plan): the
diffusivities from b at the three locations -- κ at the interfaces of the tracer columns, ν interpolated to the columns of u and of v -- and
then the three column solves read them as Fields:

  the tendencies, the diffusive calls and the AB2 steps   as in forced_model_step.py, the buoyancy flux now upwards (cooling) everywhere;
  the diffusivities and the implicit step                  κ = convective where b[k] < b[k-1], background elsewhere; then u, v, b;
  the rest                                                 as in forced_model_step.py.

The same grid, bottom, jet and stratification.  Eleven plans built once.  The step runs eagerly from a saved start, then the same chain is
captured into ONE graph and replayed from the same start: the script prints how many interfaces convect and that the two runs agree bit for
bit.
Run on an MI355X:  python examples/mixed_model_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg
from bickley_model_step import DEPTH, DT, HALO, POLE_LAT, POLE_LON, SIZE, STEPS, SUBSTEPS, bottom_height, same_bits, u_initial, v_initial
from forced_model_step import KAPPA, KAPPA_H, NU, TAU
from hydrostatic_model_step import b_initial

KAPPA_CONVECTIVE, NU_CONVECTIVE = 0.1, 0.1                         # m2/s
COOLING = 1e-5                                                     # m2/s3, upwards: strong enough to turn the top cells over within the run


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
    # a positive flux points up: a positive top flux removes buoyancy -- cooling, strongest at the equator
    stress = (-TAU * torch.cos(torch.deg2rad(3 * underlying.arrays["phi_fc"]))).contiguous()
    cooling = (COOLING * torch.cos(torch.deg2rad(underlying.arrays["phi_cc"]))).contiguous()
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
    closure = osg.ConvectiveAdjustmentVerticalDiffusivity(convective_kappa_z=KAPPA_CONVECTIVE, convective_nu_z=NU_CONVECTIVE,
                                                          background_kappa_z=KAPPA, background_nu_z=NU)
    tracer_tendency = osg.weno_tracer_advection_plan([b], u, v, w, [Gb])
    momentum_tendency = osg.momentum_advection_plan(u, v, w, Gu, Gv)
    hydrostatic = osg.hydrostatic_tendencies_plan(u, v, Gu, Gv, coriolis=coriolis, b=b, pressure=p)     # accumulates: after the advection plan
    diffusion_b = osg.diffusive_tendency_plan([b], [Gb], horizontal=osg.HorizontalScalarDiffusivity(kappa=KAPPA_H), top_flux=cooling)
    diffusion_u = osg.diffusive_tendency_plan(u, Gu, top_flux=stress)
    ab2_tracer = osg.ab2_step_plan([b], [Gb], [Gb_prev], DT, fill_halos=True)                          # the diffusivities read b beside the column
    ab2 = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gu_prev, Gv_prev, DT, GU=fs.GU, GV=fs.GV)
    implicit = osg.mixed_implicit_step_plan(closure, u, v, {"b": b}, b, DT, fill_halos=True)           # the diffusivity call, then u, v, b
    kappa = implicit.mixing.outputs["kappa_c"]
    mode = osg.barotropic_mode_plan(u, v, Ubar, Vbar)
    subcycle = osg.split_explicit_subcycle_plan(fs, DT / SUBSTEPS)
    correction = osg.barotropic_correction_plan(u, v, fs.U, fs.V, Ubar, Vbar)
    momentum_tendency()
    hydrostatic()
    tracer_tendency()
    diffusion_b()
    diffusion_u()
    for prev, now in ((Gu_prev, Gu), (Gv_prev, Gv), (Gb_prev, Gb)):
        prev.data.copy_(now.data)

    def step():
        tracer_tendency()
        momentum_tendency()
        hydrostatic()
        diffusion_b()
        diffusion_u()
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
        convecting = int((kappa.interior() == KAPPA_CONVECTIVE).sum())
        print(f"{tag}: max|u| {peak(u):.4f}, max|v| {peak(v):.4f}, max|w| {peak(w):.3e} m/s, b in [{inner(b).min().item():.5f}, "
              f"{inner(b).max().item():.5f}], {convecting} interfaces convect")

    state = [u, v, w, b, p, Gu, Gv, Gb, Gu_prev, Gv_prev, Gb_prev, Ubar, Vbar, fs.GU, fs.GV, *fs.state, *fs.twins, *fs.averages,
             *(f for f in implicit.mixing.outputs.values() if f is not None)]
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
