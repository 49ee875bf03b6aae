#!/usr/bin/env python3
"""A whole split-explicit hydrostatic step on the device (the reference's drivers build
HydrostaticFreeSurfaceModel(; grid, free_surface = SplitExplicitFreeSurface(grid; substeps = 30)): examples/bickley_jet.jl:44-55):

  the barotropic mode     Ū = Σ_k Δz u,  V̄ = Σ_k Δz v  of the predictor velocities;
  the sub-cycle           30 forward-backward sub-steps of (η, U, V), each ONE launch and the halo fill of the three fields it wrote;
  the correction          u += (U − Ū) / H,  v += (V − V̄) / H,  so that the 3-D velocities carry the sub-cycled transport;
  w from continuity.

A 1-degree tripolar grid with 10 unevenly spaced levels under an ImmersedBoundaryGrid whose bottom masks the two grid poles and the far south.
The free surface owns η, U, V, their averages and the forcing on its extended-halo grid, with_halo((Hx, substeps + 1, Hz), grid).  Four plans
built once, then per step: mode -> sub-cycle -> correction -> w; the chain is also captured into ONE graph and replayed.  The forcing Gᵁ, Gⱽ is
zero here (a model computes it from its 3-D tendencies), so the sub-cycle is a free gravity-wave adjustment of the initial bump of η.
Run on an MI355X:  python examples/split_explicit_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

SIZE = (360, 180, 10)
HALO = (5, 5, 5)
SUBSTEPS = 30
DT = 600.0                                                         # the baroclinic step; the sub-steps are DT / SUBSTEPS = 20 s
POLE_LON, POLE_LAT = 75, 35
FACES = [-1000.0, -700.0, -480.0, -320.0, -205.0, -125.0, -70.0, -35.0, -15.0, -5.0, 0.0]


def bottom_height(lam, phi):
    box = lambda lon: ((lam - lon).abs() < 5) & ((POLE_LAT - phi).abs() < 5)
    land = box(POLE_LON) | box(POLE_LON + 180) | (phi < -78)
    return torch.where(land, torch.ones_like(lam), torch.full_like(lam, FACES[0]))


def main():
    torch.cuda.set_device(0)
    underlying = osg.TripolarGrid(size=SIZE, halo=HALO, z=FACES, first_pole_longitude=POLE_LON, north_poles_latitude=POLE_LAT)
    grid = osg.ImmersedBoundaryGrid(underlying, osg.GridFittedBottom(bottom_height))
    fs = osg.SplitExplicitFreeSurface(grid, substeps=SUBSTEPS)     # η, U, V, η̄, Ū, V̄, Gᵁ, Gⱽ on the extended-halo grid, and the twins
    print(fs)
    for name in ("dx_fc", "dy_fc"):                                # the (Face, Center) nodes at the two grid poles have a zero metric, where the
        metric = fs.extended_grid.arrays[name]                     # rule divides 0 by 0; they are land here (H = 0) and a model masks them: the
        metric[metric == 0] = 1.0                                  # free surface's own grid gets a non-zero value there instead
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Ubar, Vbar = osg.Field(fs.U.loc, fs.extended_grid), osg.Field(fs.V.loc, fs.extended_grid)
    rad = torch.pi / 180
    u.set_(lambda lam, phi, z: 0.1 * (1 / torch.cosh(phi * rad * 6) ** 2 + 0 * lam) * torch.exp(z / 300))
    fs.eta.set_(lambda lam, phi, z: 0.5 * torch.exp(-((lam - 200) / 10) ** 2 - (phi / 10) ** 2))
    osg.mask_immersed_field([u, v], 0)
    osg.fill_halo_regions([fs.eta])
    mode = osg.barotropic_mode_plan(u, v, Ubar, Vbar)                                  # ONE launch for both fields, and their fill
    subcycle = osg.split_explicit_subcycle_plan(fs, DT / SUBSTEPS)                     # 30 x (ONE launch + ONE fill)
    correction = osg.barotropic_correction_plan(u, v, fs.U, fs.V, Ubar, Vbar)          # ONE launch (u, v masked in it) + their halo fill
    continuity = osg.continuity_plan(u, v, w)

    def step():
        mode()
        fs.U.data.copy_(Ubar.data)                                 # the sub-cycle starts from the barotropic mode of the predictor
        fs.V.data.copy_(Vbar.data)
        subcycle()
        correction()
        continuity()

    def report(tag):
        inner = lambda f: f.interior()[0, :-1]                     # row Ny apart: its east half is the fold's
        eta, wi = inner(fs.eta), w.interior()
        print(f"{tag}: max|η| {eta[torch.isfinite(eta)].abs().max().item():.4f} m, max|U| {inner(fs.U).abs().max().item():.3e} m2/s, "
              f"max|w| {wi[torch.isfinite(wi)].abs().max().item():.3e} m/s")

    for n in range(3):
        step()
        report(f"step {n}")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                                 # the same chain as ONE graph: nothing in it allocates
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    for n in range(3, 6):
        graph.replay()
        report(f"step {n} (graph)")


if __name__ == "__main__":
    main()
