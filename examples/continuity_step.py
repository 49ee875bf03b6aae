#!/usr/bin/env python3
"""What a hydrostatic model step runs after its velocity update: fill the halos of u and v, diagnose w from continuity, and hand all three
velocities to the time-step wizard (the reference's drivers point TimeStepWizard and the output writer at model.velocities, w included:
examples/bickley_jet.jl:75-87).  With w = 0, as a host without this operator keeps it, cell_advection_timescale quietly drops its vertical
term; here w is the real one.

A 1-degree tripolar grid with 10 unevenly spaced levels, wrapped as the reference's examples wrap theirs in an ImmersedBoundaryGrid whose
bottom height masks the two grid poles (where spacings vanish) and the far south, and a Bickley-jet-like state; two plans built once -- the
mask and halo fill of (u, v), and the continuity launch with w's mask and own fill -- then per step:
mask + fill -> w from continuity -> cell_advection_timescale(u, v, w) -> the wizard.
Run on an MI355X:  python examples/continuity_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

SIZE = (360, 180, 10)
POLE_LON, POLE_LAT = 75, 35
FACES = [-1000.0, -700.0, -480.0, -320.0, -205.0, -125.0, -70.0, -35.0, -15.0, -5.0, 0.0]


def bottom_height(lam, phi):
    box = lambda lon: ((lam - lon).abs() < 5) & ((POLE_LAT - phi).abs() < 5)
    land = box(POLE_LON) | box(POLE_LON + 180) | (phi < -78)
    return torch.where(land, torch.ones_like(lam), torch.full_like(lam, FACES[0]))


def main():
    torch.cuda.set_device(0)
    underlying = osg.TripolarGrid(size=SIZE, halo=(5, 5, 5), z=FACES, first_pole_longitude=POLE_LON, north_poles_latitude=POLE_LAT)
    grid = osg.ImmersedBoundaryGrid(underlying, osg.GridFittedBottom(bottom_height))
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    rad = torch.pi / 180
    u.set_(lambda lam, phi, z: (1 / torch.cosh(phi * rad * 6) ** 2 + 0 * lam) * torch.exp(z / 300))                  # a surface-intensified jet
    v.set_(lambda lam, phi, z: 0.1 * torch.sin(3 * lam * rad) * torch.exp(-(phi * rad * 6) ** 2) * torch.exp(z / 300))
    fill = osg.halo_fill_plan((u, v), mask_immersed=0.0)           # a model's update_state!: mask, then fill
    continuity = osg.continuity_plan(u, v, w)                      # ONE launch (w's peripheral faces masked in it) + w's halo fill; allocates nothing
    timescale = osg.advection_timescale_plan(u, v, w)
    wizard = osg.TimeStepWizard(cfl=0.2, max_dt=3600.0)
    dt = 60.0
    for step in range(3):
        fill()                                                     # the operator reads u[Nx+1, j] and v[i, Ny+1]: the periodic image and the fold
        continuity()
        tau = timescale().result()
        dt = wizard.new_time_step(dt, tau)
        wi = w.interior()
        ok = torch.isfinite(wi)
        print(f"step {step}: max|w| {wi[ok].abs().max().item():.3e} m/s over {int(ok.sum())} finite faces, advective timescale {tau:.3e} s, "
              f"next dt {dt:.1f} s")
        u.data.mul_(1.05)                                          # stand-in for the velocity update of the next step
    flat = osg.advection_timescale_plan(u, v, osg.ZFaceField(grid))().result()
    print(f"with w = 0 the timescale would read {flat:.3e} s: the vertical term is what the continuity launch adds")


if __name__ == "__main__":
    main()
