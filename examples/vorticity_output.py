#!/usr/bin/env python3
"""The output step of the reference's model drivers (examples/bickley_jet.jl:57,79; examples/distributed_bickley_jet.jl:59,83): ζ is created
with VerticalVorticityField(model) and written beside u, v and the tracer c on every output.

Here: a 1-degree tripolar grid with 10 levels, a Bickley-jet-like state (a zonal jet with a meridional perturbation, a tracer), the halos of
the state filled as a model's update_state! leaves them; then, per output, ONE plan call -- the vorticity launch and ζ's own halo fill --
and the four interiors written to one file.  Run on an MI355X:  python examples/vorticity_output.py [OUTPUT.pt]
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import orthogonalsphericalshellgrids.jl_amd as osg

SIZE = (360, 180, 10)


def main():
    torch.cuda.set_device(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(tempfile.mkdtemp(prefix="vorticity_output_"), "output.pt")
    grid = osg.TripolarGrid(size=SIZE, halo=(5, 5, 5), z=(-1000, 0))
    u, v, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    rad = torch.pi / 180
    u.set_(lambda lam, phi, z: 1 / torch.cosh(phi * rad * 6) ** 2 + 0 * lam + 0 * z)             # the jet
    v.set_(lambda lam, phi, z: 0.1 * torch.sin(3 * lam * rad) * torch.exp(-(phi * rad * 6) ** 2) + 0 * z)
    c.set_(lambda lam, phi, z: torch.sin(phi * rad) + 0 * lam + 0 * z)
    state = osg.halo_fill_plan((u, v, c))
    state()                                                        # the model state with filled halos: what the operator reads
    zeta = osg.VerticalVorticityField(u, v)
    outputs = {"u": u, "v": v, "c": c, "zeta": zeta}

    def write_output():
        osg.compute_(zeta)                                         # ONE plan call: tpg_vertical_vorticity + zeta's halo fill
        torch.save({name: f.interior().cpu() for name, f in outputs.items()}, path)

    write_output()
    z = zeta.interior()
    ok = torch.isfinite(z)
    print(f"wrote u, v, c, zeta ({tuple(z.shape)} each) to {path}")
    print(f"  zeta: min {z[ok].min().item():+.3e}  max {z[ok].max().item():+.3e} 1/s over {int(ok.sum())} finite nodes "
          f"({int((~ok).sum())} nodes sit on a grid pole, where Az = 0)")


if __name__ == "__main__":
    main()
