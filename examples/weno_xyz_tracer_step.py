#!/usr/bin/env python3
"""A tracer time-stepped end to end on the device with the advection scheme of the reference's second driver:
examples/distributed_bickley_jet.jl:50 has `tracer_advection = WENO()`, fifth-order WENO in all three directions.
weno_xyz_tracer_advection_plan computes the tendency in one launch -- WENO against the flow in x, y and z, the order of a z-face dropping
beside the bottom and the surface -- into the G that ab2_step_plan consumes.

The Bickley grid of the reference's example (here 120 x 60 with 8 levels, so that faces of every order occur; halo 5, poles at 45 / 225 E,
25 N), wrapped in an ImmersedBoundaryGrid whose bottom height masks the two grid poles and the far south, a jet with a meridional
perturbation that varies with depth, w from continuity (not zero: the horizontal flow diverges), and a tracer with a sharp front in
latitude AND in depth, which is what the upwind-biased reconstruction is for in the vertical too (the centred mean of
examples/weno_tracer_step.py is dispersive there).  Plans are built once; a step is
    tendency (one launch, the nodes under the bottom masked in it) -> ab2_step_fields (one launch) -> the tracer's halo fill
run `steps` times eagerly and, from the same start, as ONE captured graph replayed `steps` times: the two give identical bits.
Run on an MI355X:  python examples/weno_xyz_tracer_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

SIZE = (120, 60, 8)
HALO = (5, 5, 5)
POLE_LON, POLE_LAT = 45, 25
DEPTH = 1000.0
DT = 600.0


def bottom_height(lam, phi):
    box = lambda lon: ((lam - lon).abs() < 5) & ((POLE_LAT - phi).abs() < 5)
    land = box(POLE_LON) | box(POLE_LON + 180) | (phi < -78)
    return torch.where(land, torch.ones_like(lam), torch.full_like(lam, -DEPTH))


def run(size=SIZE, steps=4, quiet=False):
    """-> ({name: tensor} after `steps` eager steps, the same after `steps` replays of one graph from the same start)"""
    assert size[2] >= 6, "fewer than 6 levels have no z-face of order 5"
    torch.cuda.set_device(0)
    say = (lambda *a: None) if quiet else print
    underlying = osg.TripolarGrid(size=size, halo=HALO, z=(-DEPTH, 0), first_pole_longitude=POLE_LON, north_poles_latitude=POLE_LAT)
    grid = osg.ImmersedBoundaryGrid(underlying, osg.GridFittedBottom(bottom_height))
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, G, Gm = osg.CenterField(grid, name="c"), osg.CenterField(grid, name="Gc"), osg.CenterField(grid, name="Gc_prev")
    rad = torch.pi / 180
    u.set_(lambda lam, phi, z: 1 / torch.cosh(phi * rad * 6) ** 2 + 0 * lam + 0 * z)                                  # the Bickley jet
    v.set_(lambda lam, phi, z: 0.1 * torch.sin(3 * lam * rad) * torch.exp(-(phi * rad * 6) ** 2) * torch.cos(torch.pi * z / DEPTH))
    c.set_(lambda lam, phi, z: ((phi > 5) & (z > -DEPTH / 2)).to(lam.dtype) + 0 * lam)                                # a front at 5 N and at mid-depth
    osg.halo_fill_plan((u, v, c), mask_immersed=0.0)()             # a model's update_state!: mask, then fill -- the rule reads every halo
    osg.continuity_plan(u, v, w)()                                 # the w the vertical flux needs
    tendency = osg.weno_xyz_tracer_advection_plan([c], u, v, w, [G], scheme=osg.WENO())  # ONE launch; allocates nothing
    step = osg.ab2_step_plan([c], [G], [Gm], DT, chi=0.1, fill_halos=True)
    fields = {"c": c, "G": G, "Gm": Gm}
    start = {name: f.data.clone() for name, f in fields.items()}

    for n in range(steps):
        tendency()
        step()
        ci = c.interior()
        say(f"step {n} (eager): max|G| {G.interior().abs().max().item():.3e} 1/s, tracer in [{ci.min().item():+.6f}, {ci.max().item():+.6f}]")
    eager = {name: f.data.clone() for name, f in fields.items()}

    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tendency()
            step()
    torch.cuda.current_stream().wait_stream(side)
    for name, f in fields.items():
        f.data.copy_(start[name])
    for n in range(steps):
        graph.replay()
    torch.cuda.synchronize()
    replayed = {name: f.data.clone() for name, f in fields.items()}
    same = all(torch.equal(eager[name].view(torch.int64 if eager[name].dtype == torch.float64 else torch.int32),
                           replayed[name].view(torch.int64 if replayed[name].dtype == torch.float64 else torch.int32)) for name in fields)
    say(f"{steps} replays of one graph from the same start: identical bits: {same}")
    return eager, replayed


if __name__ == "__main__":
    run()
