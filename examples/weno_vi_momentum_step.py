#!/usr/bin/env python3
"""The closed hydrostatic model step of examples/weno_momentum_step.py with upwinding in EVERY term of the momentum advection: the
reference's drivers build their model with `momentum_advection = WENOVectorInvariant(vorticity_order = 5)` (examples/bickley_jet.jl:49).
Here u, v are advected by weno_vi_momentum_advection_plan -- weno_vi.BUILT: the WENO5 vorticity flux of that example, the upwinded
divergence flux with the WENO flux of u and v in z, and the upwinded kinetic-energy gradient; DefaultStencil smoothness of the vorticity
reconstruction is all that separates it from the drivers' scheme -- and c by weno_tracer_advection_plan.  Everything else is that
example's:

  the tendencies          Gc = -div(U c) with WENO5 faces (ONE launch), Gu, Gv upwinded in every term (ONE call for both);
  the AB2 steps           c += Δt ((1.5 + χ) Gc − (0.5 + χ) Gc⁻) and its fill; u, v likewise with Gᵁ = Σ_k Δz ĝ, Gⱽ in the same launch;
  the barotropic mode     Ū = Σ_k Δz u,  V̄ = Σ_k Δz v  of the predictor velocities;
  the sub-cycle           30 forward-backward sub-steps of (η, U, V) forced by Gᵁ, Gⱽ;
  the correction          u += (U − Ū) / H,  v += (V − V̄) / H, masked, and the fill of u, v;
  w from continuity       with its horizontal halos filled: the tendencies of the next step read them.

A small tripolar grid (120 x 60 x 4, the model halo 5: both WENO rules need at least (3, 3, 1)) under an ImmersedBoundaryGrid whose bottom masks the two grid poles and the far
south, with the Bickley jet of the reference's driver as initial condition: a sech² zonal jet plus a small vortical perturbation, and a
sinusoidal tracer.  Seven plans built once.  The step runs eagerly from a saved start, then the same chain is captured into ONE graph and
replayed from the same start: the script prints that the two agree bit for bit.
Run on an MI355X:  python examples/weno_vi_momentum_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

SIZE = (120, 60, 4)
HALO = (5, 5, 5)
SUBSTEPS = 30
DT = 300.0
STEPS = 3
POLE_LON, POLE_LAT = 75, 35
DEPTH = 1000.0
EPS, ELL, KAPPA = 0.1, 0.5, 2.5                                    # the perturbation's magnitude, Gaussian width and wavenumber


def bottom_height(lam, phi):
    box = lambda lon: ((lam - lon).abs() < 8) & ((POLE_LAT - phi).abs() < 8)                                  # noqa: E731
    land = box(POLE_LON) | box(POLE_LON + 180) | (phi < -75)
    return torch.where(land, torch.ones_like(lam), torch.full_like(lam, -DEPTH))


def psi(x, y):
    return torch.exp(-(y + ELL / 10) ** 2 / (2 * ELL ** 2)) * torch.cos(KAPPA * x) * torch.cos(KAPPA * y)


def u_initial(lam, phi, z):
    x, y = torch.deg2rad(lam) * 2, torch.deg2rad(phi) * 8
    return 1 / torch.cosh(y) ** 2 + EPS * psi(x, y) * (KAPPA * torch.tan(KAPPA * y) + y / ELL ** 2) + 0 * z


def v_initial(lam, phi, z):
    x, y = torch.deg2rad(lam) * 2, torch.deg2rad(phi) * 4
    return -EPS * psi(x, y) * KAPPA * torch.tan(KAPPA * x) + 0 * z


def c_initial(lam, phi, z):
    return torch.sin(2 * torch.pi * torch.deg2rad(phi) * 8 / 167.0) + 0 * lam + 0 * z


def same_bits(x, y):
    return bool(((x.view(torch.int64) == y.view(torch.int64)) | (x.isnan() & y.isnan())).all())


def main(momentum_plan=osg.weno_vi_momentum_advection_plan):
    """momentum_plan(u, v, w, Gu, Gv) -> the plan of Gu, Gv: examples/weno_vs_momentum_step.py passes the drivers' own scheme"""
    torch.cuda.set_device(0)
    underlying = osg.TripolarGrid(size=SIZE, halo=HALO, z=(-DEPTH, 0), first_pole_longitude=POLE_LON, north_poles_latitude=POLE_LAT)
    for name in ("dx_fc", "dy_fc", "az_fc", "az_ff"):             # the (Face, Center) / (Face, Face) nodes at the two grid poles have zero
        metric = underlying.arrays[name]                           # metrics, where the rules divide by them; they are land here and masked:
        metric[metric == 0] = 1.0                                  # a non-zero value there keeps NaN out of the neighbours' means
    grid = osg.ImmersedBoundaryGrid(underlying, osg.GridFittedBottom(bottom_height))
    fs = osg.SplitExplicitFreeSurface(grid, substeps=SUBSTEPS)
    for name in ("dx_fc", "dy_fc"):
        metric = fs.extended_grid.arrays[name]
        metric[metric == 0] = 1.0
    u, v, w, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.CenterField(grid)
    Gu, Gv, Gu_prev, Gv_prev = osg.XFaceField(grid), osg.YFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid)
    Gc, Gc_prev = osg.CenterField(grid), osg.CenterField(grid)
    Ubar, Vbar = osg.Field(fs.U.loc, fs.extended_grid), osg.Field(fs.V.loc, fs.extended_grid)
    u.set_(u_initial)
    v.set_(v_initial)
    c.set_(c_initial)
    osg.mask_immersed_field([u, v, c], 0)
    osg.fill_halo_regions([u, v, c, fs.eta])
    continuity = osg.continuity_plan(u, v, w)                      # fills w's halos by default
    continuity()
    tracer_tendency = osg.weno_tracer_advection_plan([c], u, v, w, [Gc])
    momentum_tendency = momentum_plan(u, v, w, Gu, Gv)                                # ONE call for Gu and Gv
    ab2_tracer = osg.ab2_step_plan([c], [Gc], [Gc_prev], DT, fill_halos=True)
    ab2 = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gu_prev, Gv_prev, DT, GU=fs.GU, GV=fs.GV, fill_halos=True)
    mode = osg.barotropic_mode_plan(u, v, Ubar, Vbar)
    subcycle = osg.split_explicit_subcycle_plan(fs, DT / SUBSTEPS)
    correction = osg.barotropic_correction_plan(u, v, fs.U, fs.V, Ubar, Vbar)
    momentum_tendency()                                            # the first step is Euler-like: the previous tendencies are the current ones
    tracer_tendency()
    for prev, now in ((Gu_prev, Gu), (Gv_prev, Gv), (Gc_prev, Gc)):
        prev.data.copy_(now.data)

    def step():
        tracer_tendency()
        momentum_tendency()
        ab2_tracer()
        ab2()
        mode()
        fs.U.data.copy_(Ubar.data)                                 # the sub-cycle starts from the barotropic mode of the predictor
        fs.V.data.copy_(Vbar.data)
        subcycle()
        correction()
        continuity()

    def report(tag):
        inner = lambda f: f.interior()[..., :-1, :]                # row Ny apart: its east half is the fold's                # noqa: E731
        peak = lambda f: inner(f)[torch.isfinite(inner(f))].abs().max().item()                                                 # noqa: E731
        print(f"{tag}: max|u| {peak(u):.4f}, max|v| {peak(v):.4f}, max|w| {peak(w):.3e} m/s, max|Gu| {peak(Gu):.3e} m/s2, "
              f"max|η| {peak(fs.eta):.4f} m, c in [{inner(c).min().item():.4f}, {inner(c).max().item():.4f}]")

    state = [u, v, w, c, Gu, Gv, Gc, Gu_prev, Gv_prev, Gc_prev, Ubar, Vbar, fs.GU, fs.GV, *fs.state, *fs.twins, *fs.averages]
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
    finite = all(bool(torch.isfinite(f.interior()[..., :-1, :]).all()) for f in (u, v, c, Gu, Gv))
    print(f"eager and replayed graph agree bit for bit on all {len(state)} fields: {agree}; u, v, c, Gu, Gv finite below row Ny: {finite}")
    assert agree


if __name__ == "__main__":
    main()
