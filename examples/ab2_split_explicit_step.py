#!/usr/bin/env python3
"""A whole split-explicit hydrostatic step on the device WITH its head: the quasi-Adams-Bashforth-2 step that turns the 3-D tendencies into
predictor velocities and into the forcing Gᵁ, Gⱽ of the free surface's sub-cycle (the reference's drivers build
HydrostaticFreeSurfaceModel(; grid, free_surface = SplitExplicitFreeSurface(grid; substeps = 30)): examples/bickley_jet.jl:44-55):

  the AB2 step            u += Δt ((1.5 + χ) Gu − (0.5 + χ) Gu⁻),  Gu⁻ = Gu,  Gᵁ = Σ_k Δz ĝ  (v, Gⱽ likewise): ONE launch, then the fill of u, v;
  the barotropic mode     Ū = Σ_k Δz u,  V̄ = Σ_k Δz v  of the predictor velocities;
  the sub-cycle           30 forward-backward sub-steps of (η, U, V) forced by Gᵁ, Gⱽ, each ONE launch and the halo fill of what it wrote;
  the correction          u += (U − Ū) / H,  v += (V − V̄) / H,  so that the 3-D velocities carry the sub-cycled transport;
  w from continuity.

A 1-degree tripolar grid with 10 unevenly spaced levels under an ImmersedBoundaryGrid whose bottom masks the two grid poles and the far south.
The tendencies stand in for a model's (the advective ones are examples/bickley_model_step.py's; Coriolis and the pressure gradient are out
of scope): a steady zonal wind stress spread
over the upper 70 m.  Five plans built once, then per step: AB2 -> mode -> sub-cycle -> correction -> w.  The step runs eagerly from a saved
start, then the same chain is captured into ONE graph and replayed from the same start: the script prints that the two agree bit for bit.
Run on an MI355X:  python examples/ab2_split_explicit_step.py
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
STEPS = 3
POLE_LON, POLE_LAT = 75, 35
FACES = [-1000.0, -700.0, -480.0, -320.0, -205.0, -125.0, -70.0, -35.0, -15.0, -5.0, 0.0]


def bottom_height(lam, phi):
    box = lambda lon: ((lam - lon).abs() < 5) & ((POLE_LAT - phi).abs() < 5)
    land = box(POLE_LON) | box(POLE_LON + 180) | (phi < -78)
    return torch.where(land, torch.ones_like(lam), torch.full_like(lam, FACES[0]))


def same_bits(x, y):
    return bool(((x.view(torch.int64) == y.view(torch.int64)) | (x.isnan() & y.isnan())).all())


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
    Gu, Gv, Gu_prev, Gv_prev = osg.XFaceField(grid), osg.YFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid)
    Ubar, Vbar = osg.Field(fs.U.loc, fs.extended_grid), osg.Field(fs.V.loc, fs.extended_grid)
    rad = torch.pi / 180
    u.set_(lambda lam, phi, z: 0.1 * (1 / torch.cosh(phi * rad * 6) ** 2 + 0 * lam) * torch.exp(z / 300))
    Gu.set_(lambda lam, phi, z: 1e-6 * (torch.cos(phi * rad * 3) + 0 * lam) * (z > -70))      # 0.1 N/m2 over 70 m of 1e3 kg/m3, per second
    Gu_prev.data.copy_(Gu.data)
    fs.eta.set_(lambda lam, phi, z: 0.5 * torch.exp(-((lam - 200) / 10) ** 2 - (phi / 10) ** 2))
    osg.mask_immersed_field([u, v], 0)
    osg.fill_halo_regions([fs.eta])
    ab2 = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gu_prev, Gv_prev, DT, GU=fs.GU, GV=fs.GV, fill_halos=True)   # ONE launch, both fields and planes
    mode = osg.barotropic_mode_plan(u, v, Ubar, Vbar)                                  # ONE launch for both fields, and their fill
    subcycle = osg.split_explicit_subcycle_plan(fs, DT / SUBSTEPS)                     # 30 x (ONE launch + ONE fill)
    correction = osg.barotropic_correction_plan(u, v, fs.U, fs.V, Ubar, Vbar)          # ONE launch (u, v masked in it) + their halo fill
    continuity = osg.continuity_plan(u, v, w)

    def step():
        ab2()                                                      # a model computes Gu, Gv first; here they are steady
        mode()
        fs.U.data.copy_(Ubar.data)                                 # the sub-cycle starts from the barotropic mode of the predictor
        fs.V.data.copy_(Vbar.data)
        subcycle()
        correction()
        continuity()

    def report(tag):
        inner = lambda f: f.interior()[0, :-1]                     # row Ny apart: its east half is the fold's
        eta, wi, gu = inner(fs.eta), w.interior(), inner(fs.GU)
        print(f"{tag}: max|η| {eta[torch.isfinite(eta)].abs().max().item():.4f} m, max|U| {inner(fs.U).abs().max().item():.3e} m2/s, "
              f"max|Gᵁ| {gu.abs().max().item():.3e} m2/s2, max|w| {wi[torch.isfinite(wi)].abs().max().item():.3e} m/s")

    state = [u, v, w, Gu_prev, Gv_prev, Ubar, Vbar, fs.GU, fs.GV, *fs.state, *fs.twins, *fs.averages]
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
    # the wizard changes Δt: the plan over the same tensors with the new step; a captured graph is re-captured then
    ab2 = ab2.with_dt(DT / 2)
    assert ab2.dt == DT / 2 and agree


if __name__ == "__main__":
    main()
