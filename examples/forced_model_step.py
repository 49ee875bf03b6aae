#!/usr/bin/env python3
"""examples/vertical_diffusion_model_step.py with something acting on the ocean from outside, and the dissipation the centred and WENO
tracer tendencies lack:

  a wind stress            a (Face, Center) plane through u's top face;
  a surface buoyancy flux  a (Center, Center) plane through b's top face;
  horizontal diffusion     `HorizontalScalarDiffusivity(κ = 10)` of b, explicit.

Boundary fluxes enter the EXPLICIT tendency (the implicit step leaves the faces 1 and Nz + 1 without flux on purpose), so the step gains TWO
launches (diffusive_tendency_plan), ADDed to Gu and Gb after the advection and hydrostatic calls and before AB2:

  the tendencies          as in hydrostatic_model_step.py, then the diffusive calls: b with κ_h and its surface flux, the faces between wet
                          and dry cells closed; u with its wind stress alone (a vertical-only call with az_fc and the (Face, Center) counts);
  the AB2 steps, the implicit step and the rest   as in vertical_diffusion_model_step.py.

The same grid, bottom, jet and stratification.  Eleven plans built once.  The step runs eagerly from a saved start, then the same chain is
captured into ONE graph and replayed from the same start: the script prints that the two agree bit for bit.
Run on an MI355X:  python examples/forced_model_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg
from bickley_model_step import DEPTH, DT, HALO, POLE_LAT, POLE_LON, SIZE, STEPS, SUBSTEPS, bottom_height, same_bits, u_initial, v_initial
from hydrostatic_model_step import b_initial

NU, KAPPA, KAPPA_H = 1e-2, 1e-4, 10.0                              # m2/s
TAU, JB = 1e-4, 1e-8                                               # m2/s2 (a stress over the density), m2/s3


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
    # a positive flux points up: a positive top flux removes.  Eastward wind in the tropics, westward at mid-latitudes; buoyancy in at the equator
    stress = (-TAU * torch.cos(torch.deg2rad(3 * underlying.arrays["phi_fc"]))).contiguous()
    heating = (-JB * torch.cos(torch.deg2rad(underlying.arrays["phi_cc"]))).contiguous()
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
    # accumulates, with b's surface flux; then u's wind stress alone.  The planes go to the plans: this grid has fewer levels than halo planes
    # (Nz < Hz), where the halo fill takes no explicit top condition; with Nz >= Hz they can be the fields' own FluxBoundaryCondition
    diffusion_b = osg.diffusive_tendency_plan([b], [Gb], horizontal=osg.HorizontalScalarDiffusivity(kappa=KAPPA_H), top_flux=heating)
    diffusion_u = osg.diffusive_tendency_plan(u, Gu, top_flux=stress)
    ab2_tracer = osg.ab2_step_plan([b], [Gb], [Gb_prev], DT)
    ab2 = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gu_prev, Gv_prev, DT, GU=fs.GU, GV=fs.GV)
    implicit = osg.implicit_step_plan(u, v, {"b": b}, closure, DT, fill_halos=True)                        # the fills the AB2 plans had
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
