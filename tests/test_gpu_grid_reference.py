"""tpg_build_grid against tests/grid_ref.py, the whole-array long-double statement of the reference's Julia text: every cell of every padded
parent of the kernel's 20 arrays within the tolerance derived there (Float64 arithmetic; Float32: half an ulp more), and every halo cell bit
for bit the fill of the array's own interior.  Bit parity with the oracle stays in tests/test_gpu_grid.py; this one does not load the oracle.

Shapes (grid_ref.GPU_SIZES): k_cells_tile emits 62 columns x 7 cell rows per block -- Nx and Ny on both sides of one and of two tile edges in
each direction, Nx = 0 and 2 mod 4 (the row-Ny substitution is visible only for 2 mod 4), and with the four halos both south paths: k_south
as a launch of its own (Ny <= 2 Hy + 2) and merged.  Each case builds one tiny grid."""
import numpy as np
import pytest
import torch

import grid_ref as G
from test_gpu_variants import knob  # noqa: F401  (the test library's knob fixture)

pytestmark = pytest.mark.gpu
CASES = G.gpu_cases()
TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}


def _arrays(grid):
    return {n: getattr(grid, n).cpu().numpy() for n in G.COORDS + G.METRICS}


def _build(osg, size, halo, pid, dtype, arch=None):
    return osg.TripolarGrid(arch if arch is not None else osg.GPU(0), TORCH[np.dtype(dtype)], size=size + (1,), halo=halo, **G.PARAMS[pid])


def _check(osg, case):
    size, halo, pid, dtype = case
    got = _arrays(_build(osg, size, halo, pid, dtype))
    ref = G.build(size, halo, dtype=dtype, stored=got, **G.PARAMS[pid])
    print(G.case_id(case), {k: round(v, 3) for k, v in ref.worst(got).items()})
    ref.check(got, G.case_id(case))
    G.check_halo_copies(got, size, halo)


@pytest.mark.parametrize("case", CASES, ids=[G.case_id(c) for c in CASES])
def test_kernel_within_tolerance_of_the_reference_on_every_cell(osg, gpu, case):
    _check(osg, case)


@pytest.mark.parametrize("halo,R", [((4, 4, 4), 2), ((4, 4, 4), 3), ((5, 5, 5), 6)], ids=["R2", "R3", "R6-thinner-than-Hy5"])
@pytest.mark.parametrize("dtype", G.DTYPES, ids=["f64", "f32"])
def test_latitude_bands(osg, gpu, halo, R, dtype):
    """every rank's band, built through jstart / jend, against rows jstart - Hy .. jend + Hy of the global reference
    (distributed_tripolar_grid.jl:41-49); with R = 6 the bands of 3 rows are thinner than the halo of 5"""
    size = (128, 22)
    ref = G.build(size, halo, dtype=dtype, stored=_arrays(_build(osg, size, halo, "default", dtype)))
    for r in range(R):
        band = _build(osg, size, halo, "default", dtype, osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r))
        j0, j1 = band.jrange
        assert R != 6 or r == R - 1 or j1 - j0 + 1 < halo[1]
        ref.rows(j0, j1).check(_arrays(band), f"rank {r} of {R}: rows {j0}..{j1}")


@pytest.mark.parametrize("case", [((126, 15), (4, 4, 4), "default", np.float64), ((128, 22), (3, 2, 1), "fpl1000.5", np.float32)],
                         ids=lambda c: G.case_id(c))
def test_thread_per_cell_variant(osg, gpu, knob, case):
    """TPG_CELLS_VARIANT = 0: the simple build kernel the tile kernel is checked against, itself held to the reference"""
    knob["TPG_CELLS_VARIANT"] = "0"
    osg._lib.lib().tpg_reload_config()
    _check(osg, case)
