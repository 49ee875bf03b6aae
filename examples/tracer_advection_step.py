#!/usr/bin/env python3
"""A tracer time-stepped end to end on the device: tendency -> AB2 -> halo fill.  Both of the reference's drivers carry a tracer
(`tracers = :c`, examples/bickley_jet.jl:48-55); with `buoyancy = nothing` and no closure its only tendency is minus the divergence of its
advective flux, which tracer_advection_plan computes in one launch, second-order centered, into the G that ab2_step_plan consumes.

The Bickley grid of the reference's example (180 x 90, halo 5, poles at 45 / 225 E, 25 N; here with 4 levels), wrapped in an
ImmersedBoundaryGrid whose bottom height masks the two grid poles and the far south, a jet with a meridional perturbation, w from continuity,
and a tracer that is a sine of latitude.  Plans are built once; a step is
    tendency (one launch, the nodes under the bottom masked in it) -> ab2_step_fields (one launch) -> the tracer's halo fill
first eagerly, then as ONE captured graph replayed.  The velocities are frozen, so the flow is non-divergent with its w and a constant
tracer would stay constant; the total tracer content is printed each step.
Run on an MI355X:  python examples/tracer_advection_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

SIZE = (180, 90, 4)
POLE_LON, POLE_LAT = 45, 25
DEPTH = 1000.0
DT = 600.0


def bottom_height(lam, phi):
    box = lambda lon: ((lam - lon).abs() < 5) & ((POLE_LAT - phi).abs() < 5)
    land = box(POLE_LON) | box(POLE_LON + 180) | (phi < -78)
    return torch.where(land, torch.ones_like(lam), torch.full_like(lam, -DEPTH))


def main():
    torch.cuda.set_device(0)
    underlying = osg.TripolarGrid(size=SIZE, halo=(5, 5, 5), z=(-DEPTH, 0), first_pole_longitude=POLE_LON, north_poles_latitude=POLE_LAT)
    grid = osg.ImmersedBoundaryGrid(underlying, osg.GridFittedBottom(bottom_height))
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, G, Gm = osg.CenterField(grid, name="c"), osg.CenterField(grid, name="Gc"), osg.CenterField(grid, name="Gc_prev")
    rad = torch.pi / 180
    u.set_(lambda lam, phi, z: 1 / torch.cosh(phi * rad * 6) ** 2 + 0 * lam + 0 * z)                                  # the Bickley jet
    v.set_(lambda lam, phi, z: 0.1 * torch.sin(3 * lam * rad) * torch.exp(-(phi * rad * 6) ** 2) + 0 * z)
    c.set_(lambda lam, phi, z: torch.sin(phi * rad) + 0 * lam + 0 * z)
    osg.halo_fill_plan((u, v, c), mask_immersed=0.0)()             # a model's update_state!: mask, then fill -- the rule reads every halo
    osg.continuity_plan(u, v, w)()                                 # the w the vertical flux needs
    tendency = osg.tracer_advection_plan([c], u, v, w, [G])        # ONE launch; allocates nothing
    first = osg.ab2_step_plan([c], [G], [Gm], DT, chi=-0.5, euler=True, fill_halos=True)     # a first step: the factor 1.5 + chi is one
    step = osg.ab2_step_plan([c], [G], [Gm], DT, chi=0.1, fill_halos=True)

    g = grid.underlying_grid
    (Nx, Ny, Nz), (Hx, Hy, Hz) = SIZE, (5, 5, 5)
    volume = g.arrays["az_cc"][Hy:Hy + Ny, Hx:Hx + Nx][None] * osg.z_center_spacings(grid).to(c.data.device)[:, None, None]
    wet = torch.arange(1, Nz + 1, device=c.data.device)[:, None, None] > grid.column_counts["cc"][None]

    def content():
        return float((c.interior() * volume)[wet].sum())

    start = content()
    tendency(); first()
    print(f"step 0 (Euler): max|G| {G.interior().abs().max().item():.3e} 1/s, tracer content {content() / start:.12f} of the start")
    for n in range(1, 4):
        tendency(); step()
        print(f"step {n} (eager): max|G| {G.interior().abs().max().item():.3e} 1/s, tracer content {content() / start:.12f} of the start")
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tendency()
            step()
    torch.cuda.current_stream().wait_stream(side)
    for n in range(4, 8):
        graph.replay()
    torch.cuda.synchronize()
    ci = c.interior()
    print(f"steps 4 - 7 (one graph, replayed): tracer in [{ci.min().item():.4f}, {ci.max().item():.4f}], content {content() / start:.12f} of the start, "
          f"all finite: {bool(torch.isfinite(ci).all())}")


if __name__ == "__main__":
    main()
