#!/usr/bin/env python3
"""The closed hydrostatic model step of examples/weno_vi_momentum_step.py with the momentum advection the reference's drivers name:
`momentum_advection = WENOVectorInvariant(vorticity_order = 5)` (examples/bickley_jet.jl:49, examples/distributed_bickley_jet.jl:51).
u, v are advected by weno_vs_momentum_advection_plan -- weno_vs.BUILT: upwinding in every term as in that example, with the smoothness of
the WENO5 vorticity reconstruction measured on the velocities (VelocityStencil).  Everything else -- the grid, the Bickley jet, the tracer,
the AB2 steps, the barotropic mode, the sub-cycle, the correction, w from continuity, the eager run and the ONE replayed graph, which must
agree bit for bit -- is that example's, run through its main().
Run on an MI355X:  python examples/weno_vs_momentum_step.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import orthogonalsphericalshellgrids.jl_amd as osg
from orthogonalsphericalshellgrids.jl_amd import weno_vs

import weno_vi_momentum_step


def momentum_plan(u, v, w, Gu, Gv):
    return osg.weno_vs_momentum_advection_plan(u, v, w, Gu, Gv, scheme=weno_vs.BUILT)     # ONE call for Gu and Gv


if __name__ == "__main__":
    print("momentum advection:", weno_vs._BUILT_NAME)
    weno_vi_momentum_step.main(momentum_plan)
