#!/usr/bin/env python3
"""examples/bickley_jet.jl:9-29 of the reference on this host: the 180 x 90 x 1 tripolar grid with halo (5, 5, 5) and poles at 45 / 225 E,
25 N, wrapped at once in an ImmersedBoundaryGrid whose bottom height "masks the singularities" -- the two 5-degree pole boxes and the
cap south of 78 S.  Then what a model does every step before it fills halos: mask_immersed_field! on (u, v, c), followed by
fill_halo_regions!.  Prints the masked counts.  Run on an MI355X:  python examples/bickley_mask.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

Nx, Ny = 180, 90
first_pole_longitude = lp = 45
north_poles_latitude = pp = 25
lp2 = lp + 180


def bottom_height(lam, phi):
    land = (((lam - lp).abs() < 5) & ((pp - phi).abs() < 5)) | (((lam - lp2).abs() < 5) & ((pp - phi).abs() < 5)) | (phi < -78)
    return torch.where(land, torch.ones_like(lam), torch.zeros_like(lam))


def main():
    torch.cuda.set_device(0)
    underlying_grid = osg.TripolarGrid(size=(Nx, Ny, 1), halo=(5, 5, 5), first_pole_longitude=first_pole_longitude,
                                       north_poles_latitude=north_poles_latitude)
    grid = osg.ImmersedBoundaryGrid(underlying_grid, osg.GridFittedBottom(bottom_height))
    print(grid)
    u, v, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    for f in (u, v, c):
        osg.set_(f, 1)
    plan = osg.halo_fill_plan([u, v, c], mask_immersed=0.0)       # mask, then fill: one plan, built once, run every step
    plan()
    torch.cuda.synchronize()
    counts = grid.column_counts
    phi = underlying_grid.interior("phi_cc")
    land = counts["cc"] == 1
    print(f"immersed cells: {int(land.sum())} of {Nx * Ny}  (pole boxes {int((land & (phi > 0)).sum())}, southern cap {int((land & (phi < 0)).sum())})")
    for name, f, key in (("u", u, "fc"), ("v", v, "cf"), ("c", c, "cc")):
        masked = int((osg.interior(f) == 0).sum())
        print(f"{name}: {masked} masked nodes (count plane {key}: {int(counts[key].sum())})")
    row = osg.interior(grid.immersed_boundary.bottom_height)[0, Ny - 1]
    print("row Ny of bottom_height mirror-symmetric:", bool(torch.equal(row, row.flip(0))))


if __name__ == "__main__":
    main()
