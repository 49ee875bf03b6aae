#!/usr/bin/env python3
"""The two places where a split-explicit hydrostatic step crosses between its 3-D velocities and the free surface's 2-D fields (the reference's
drivers build HydrostaticFreeSurfaceModel(; grid, free_surface = SplitExplicitFreeSurface(grid; substeps = 30)): examples/bickley_jet.jl:44-55):

  before the sub-cycle   the barotropic mode  Ū = Σ_k Δz u,  V̄ = Σ_k Δz v  of the predictor velocities;
  after the sub-cycle    the correction  u += (U − Ū) / H,  v += (V − V̄) / H,  so that the 3-D velocities carry the sub-cycled transport,
                         before w is diagnosed from continuity.

A 1-degree tripolar grid with 10 unevenly spaced levels under an ImmersedBoundaryGrid whose bottom masks the two grid poles and the far south;
U, V, Ū, V̄ on the free surface's extended-halo grid, with_halo((Hx, substeps + 1, Hz), grid).  Three plans built once -- the mode, the
correction (masking u, v and filling their halos in the same chain), w from continuity -- then per step:
mode -> [the model's sub-cycle: here a stand-in that nudges U, V] -> correction -> w.  The check printed at the end is the point of the
correction: the barotropic mode of the corrected velocities is the sub-cycled transport, to rounding.
Run on an MI355X:  python examples/barotropic_correction_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

SIZE = (360, 180, 10)
HALO = (5, 5, 5)
SUBSTEPS = 30
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
    extended = osg.with_halo((HALO[0], SUBSTEPS + 1, HALO[2]), underlying)             # the free surface's grid
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    at_u, at_v = (osg.Face, osg.Center, None), (osg.Center, osg.Face, None)
    U, V, Ubar, Vbar = osg.Field(at_u, extended), osg.Field(at_v, extended), osg.Field(at_u, extended), osg.Field(at_v, extended)
    rad = torch.pi / 180
    u.set_(lambda lam, phi, z: (1 / torch.cosh(phi * rad * 6) ** 2 + 0 * lam) * torch.exp(z / 300))
    v.set_(lambda lam, phi, z: 0.1 * torch.sin(3 * lam * rad) * torch.exp(-(phi * rad * 6) ** 2) * torch.exp(z / 300))
    osg.mask_immersed_field([u, v], 0)
    mode = osg.barotropic_mode_plan(u, v, Ubar, Vbar, fill_halos=False)                # ONE launch for both fields
    correction = osg.barotropic_correction_plan(u, v, U, V, Ubar, Vbar)                # ONE launch (u, v masked in it) + their halo fill
    continuity = osg.continuity_plan(u, v, w)
    check = osg.barotropic_mode_plan(u, v, fill_halos=False)                           # its own planes, on u's grid
    print(f"column depth by immersed count: {[round(float(h), 1) for h in osg.column_depth_table(grid)]}")
    for step in range(3):
        mode()
        U.data.copy_(Ubar.data).mul_(1.02)                         # stand-in for 30 barotropic sub-steps
        V.data.copy_(Vbar.data).mul_(0.98)
        correction()
        continuity()
        check()
        inner = lambda f: f.interior()[0, :-1]                     # row Ny apart: its east half is the fold's, written by the halo fill of u
        wet = torch.isfinite(inner(check.U)) & (inner(Ubar) != 0)
        gap = ((inner(check.U) - inner(U)).abs()[wet] / inner(U).abs()[wet].clamp_min(1e-30)).max().item()
        wi = w.interior()
        print(f"step {step}: max|Ū| {inner(Ubar).abs().max().item():.3e} m2/s, mode of the corrected u against U: {gap:.1e} relative, "
              f"max|w| {wi[torch.isfinite(wi)].abs().max().item():.3e} m/s")


if __name__ == "__main__":
    main()
