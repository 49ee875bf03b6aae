"""Host-side tests of the device reductions (no GPU): the numpy reference of tests/reduction_ref.py on hand-made cases, the three C
symbols (declared, exported, bound), tpg_reduce_workspace_bytes, every argument error of tpg_field_extrema / tpg_cell_advection_timescale
(status and message, no device work: every call below fails in validation, none reaches a launch), the time-step wizard's arithmetic and
the host rule of the z face spacings."""
import ctypes as C
import math

import numpy as np
import pytest

from immersed_ref import column_counts, inactive_cells
from reduction_ref import (cell_advection_timescale, cell_timescales, excluded_from_plane, excluded_nodes, field_extrema, same)


# ---- the reference on hand-made cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_extrema_count_the_interior_only_and_propagate_nan(dtype):
    size, halo = (4, 3, 2), (2, 1, 1)
    p = np.full((4, 5, 8), 1e30, dtype=dtype)                      # every halo cell huge
    p[1:3, 1:4, 2:6] = np.arange(24, dtype=dtype).reshape(2, 3, 4) - 5
    assert field_extrema(p, size, halo) == (-5.0, 18.0, 18.0)
    p[1, 1, 2] = -40
    assert field_extrema(p, size, halo) == (-40.0, 18.0, 40.0)
    q = p.copy()
    q[0, 0, 0] = np.nan                                            # a NaN halo cell counts for nothing
    assert field_extrema(q, size, halo) == (-40.0, 18.0, 40.0)
    q[2, 3, 5] = np.nan                                            # the last interior cell
    assert all(np.isnan(x) for x in field_extrema(q, size, halo))
    none = np.ones((2, 3, 4), dtype=bool)
    assert field_extrema(q, size, halo, none) == (np.inf, -np.inf, -np.inf)
    only = ~none
    only[1, 2, 3] = True                                           # the NaN cell left out
    assert field_extrema(q, size, halo, only) == (-40.0, 17.0, 40.0)
    assert same(np.nan, np.nan) and same(0.0, -0.0) and not same(1.0, np.nextafter(1.0, 2)) and not same(np.nan, 1.0)


def test_excluded_sets_from_the_predicate_and_from_the_count_planes_agree():
    rng = np.random.default_rng(3)
    for size, halo, wall in (((8, 6, 3), (2, 2, 1), True), ((12, 5, 4), (1, 1, 2), False)):
        Nx, Ny, Nz = size
        zc = ((np.arange(Nz) + 0.5) / Nz)
        h = rng.uniform(-0.2, 1.2, (Ny + 2 * halo[1], Nx + 2 * halo[0]))
        ina = inactive_cells(h, zc, size, halo, wall)
        n = column_counts(h, zc, size, halo, wall)
        for xl in (0, 1):
            for yl in (0, 1):
                plane = n["cf"[xl] + "cf"[yl]]
                assert np.array_equal(excluded_nodes(ina, (xl, yl, 0), size), excluded_from_plane(plane, 0, Nz))
                face = excluded_nodes(ina, (xl, yl, 1), size)
                assert face.shape == (Nz + 1, Ny, Nx) and not face[Nz].any()       # a z-Face field's top level is counted
                assert np.array_equal(face, excluded_from_plane(plane, 1, Nz + 1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_timescale_rule_on_hand_made_cells(dtype):
    size, halo = (2, 2, 2), (1, 1, 1)
    shape, wshape = (4, 4, 4), (5, 4, 4)
    u, v, w = np.zeros(shape, dtype), np.zeros(shape, dtype), np.zeros(wshape, dtype)
    dx, dy, dz = np.full((4, 4), 4, dtype), np.full((4, 4), 8, dtype), np.array([2, 0.5], dtype)
    assert cell_advection_timescale(u, v, w, dx, dy, dz, size, halo) == np.inf
    u[1, 1, 1] = -2                                                # s = 2 / 4
    assert cell_advection_timescale(u, v, w, dx, dy, dz, size, halo) == 2.0
    w[2, 2, 2] = 1                                                 # level 2: s = 1 / 0.5
    assert cell_advection_timescale(u, v, w, dx, dy, dz, size, halo) == 0.5
    w[3, 1, 1] = 1e6                                               # w's level Nz + 1 is not read
    u[0, 1, 1] = v[1, 0, 1] = 1e6                                  # nor any halo cell
    assert cell_advection_timescale(u, v, w, dx, dy, dz, size, halo) == 0.5
    v[2, 2, 2] = 4                                                 # same cell: 0 / 4 + 4 / 8 + 1 / 0.5, left to right in the field type
    tau = cell_timescales(u, v, w, dx, dy, dz, size, halo)
    assert tau.dtype == dtype and tau[1, 1, 1] == dtype(1) / (dtype(0) / dtype(4) + dtype(4) / dtype(8) + dtype(1) / dtype(0.5))
    ncc = np.array([[0, 0], [0, 2]], dtype=np.int32)               # that column immersed at both levels
    assert cell_advection_timescale(u, v, w, dx, dy, dz, size, halo, ncc) == 2.0
    assert cell_advection_timescale(u, v, w, dx, dy, dz, size, halo, np.full((2, 2), 2, np.int32)) == np.inf
    w[2, 1, 1] = np.nan
    assert np.isnan(cell_advection_timescale(u, v, w, dx, dy, dz, size, halo))
    thirds = np.full(shape, 1, dtype)                              # a value the two types round differently
    t = cell_advection_timescale(thirds, np.zeros_like(v), np.zeros_like(w), np.full((4, 4), 3, dtype), dy, dz, size, halo)
    assert t == np.float64(dtype(1) / (dtype(1) / dtype(3)))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
NAMES = ["tpg_reduce_workspace_bytes", "tpg_field_extrema", "tpg_cell_advection_timescale"]


def test_the_three_symbols_are_declared_exported_and_bound(osg):
    from test_abi import declared_symbols, exported_symbols
    lib = osg._lib.lib()
    for n in NAMES:
        assert n in declared_symbols() and n in exported_symbols(osg._lib.LIB_PATH) and n in osg._lib.SIGNATURES and hasattr(lib, n)
    assert lib.tpg_version() == 600 and len(declared_symbols()) == 38
    for name in ("field_extrema", "minimum", "maximum", "extrema_plan", "cell_advection_timescale", "advection_timescale_plan",
                 "TimeStepWizard", "minimum_xspacing", "minimum_yspacing", "grid_summary", "summary", "z_face_spacings"):
        assert hasattr(osg, name), name


def test_workspace_bytes_are_positive_and_non_decreasing(osg):
    ws = osg._lib.lib().tpg_reduce_workspace_bytes
    base = (1, 10, 10, 1)
    assert ws(*base) > 0 and ws(1, 2, 1, 1) > 0
    for axis in range(4):
        prev = 0
        for value in (1, 2, 3, 7, 16, 17, 64, 75, 100, 1800, 3600, 100000):
            args = list(base)
            args[axis] = value if axis != 1 else 2 * value
            got = ws(*args)
            assert got >= prev and got > 0, (axis, value)
            prev = got
    assert ws(4, 3600, 1800, 75) >= 4 * ws(1, 3600, 1800, 75) > 0
    assert ws(4, 3600, 1800, 75) < 1 << 20                          # one partial per block, not per row


def test_argument_errors_without_device_work(osg):
    lib = osg._lib.lib()
    P = 1 << 20                                                    # a non-NULL pointer that is never dereferenced
    err = lambda: lib.tpg_last_error().decode()
    good, null_field = (C.c_void_p * 1)(P), (C.c_void_p * 1)(None)
    planes, zl = (C.c_void_p * 1)(P), (C.c_int8 * 1)(0)
    g3 = (48, 40, 3, 4, 4, 4)
    big = 1 << 30
    ext = lambda *a: lib.tpg_field_extrema(*a)
    assert ext(good, 1, planes, zl, P, P, big, *g3, 7, None) == -1 and err() == "unknown element type ft=7"
    assert ext(good, 1, planes, zl, P, P, big, 49, 40, 3, 4, 4, 4, 1, None) == -2
    assert ext(good, 0, planes, zl, P, P, big, *g3, 1, None) == -1 and err() == "no fields"
    assert ext(None, 1, planes, zl, P, P, big, *g3, 1, None) == -1 and err() == "no fields"
    assert ext(null_field, 1, planes, zl, P, P, big, *g3, 1, None) == -1 and err() == "null field 0"
    assert ext(good, 1, planes, None, P, P, big, *g3, 1, None) == -1 and err() == "a counts table needs a zloc table"
    for bad in (2, -1):
        assert ext(good, 1, planes, (C.c_int8 * 1)(bad), P, P, big, *g3, 1, None) == -1 and "neither TPG_CENTER nor TPG_FACE" in err()
    assert ext((C.c_void_p * 1)(P + 4), 1, None, None, P, P, big, *g3, 1, None) == -1 and err() == "field 0: pointer not aligned to its element type"
    assert ext((C.c_void_p * 1)(P + 2), 1, None, None, P, P, big, *g3, 0, None) == -1 and err() == "field 0: pointer not aligned to its element type"
    assert ext(good, 1, (C.c_void_p * 1)(P + 2), zl, P, P, big, *g3, 1, None) == -1 and err() == "field 0: count plane pointer not aligned to int32"
    assert ext(good, 1, None, None, None, P, big, *g3, 1, None) == -1 and err() == "null out"
    assert ext(good, 1, None, None, P + 4, P, big, *g3, 1, None) == -1 and err() == "out pointer not aligned to double"
    assert ext(good, 1, None, None, P, P, big, 2, 65536, 32768, 0, 0, 0, 1, None) == -5 and "32-bit" in err()
    assert ext(good, 1, None, None, P, None, big, *g3, 1, None) == -4 and err().startswith("null workspace")
    assert ext(good, 1, None, None, P, P + 4, big, *g3, 1, None) == -4 and err() == "workspace not 8-B aligned"
    need = lib.tpg_reduce_workspace_bytes(1, 48, 40, 3)
    assert ext(good, 1, None, None, P, P, need - 1, *g3, 1, None) == -4 and err().startswith("workspace too small")
    assert ext(good, 1, None, None, P, P, 0, *g3, 1, None) == -4
    # a fault in the SECOND batch of a table is found before the first batch is launched; so is a workspace sized for 16 of 17 fields
    n = 17
    many = (C.c_void_p * n)(*([P] * n))
    assert ext(many, n, many, (C.c_int8 * n)(*([0] * 16 + [5])), P, P, big, *g3, 1, None) == -1 and err().startswith("field 16: zloc = 5")
    assert ext(many, n, None, None, P, P, lib.tpg_reduce_workspace_bytes(16, 48, 40, 3), *g3, 1, None) == -4

    tau = lambda *a: lib.tpg_cell_advection_timescale(*a)
    six = (P,) * 6
    assert tau(*six, None, P, P, big, *g3, 7, None) == -1 and err() == "unknown element type ft=7"
    assert tau(*six, None, P, P, big, 49, 40, 3, 4, 4, 4, 1, None) == -2
    for q in range(3):
        a = list(six)
        a[q] = None
        assert tau(*a, None, P, P, big, *g3, 1, None) == -1 and err() == "null u, v or w"
        a = list(six)
        a[q] = P + 4
        assert tau(*a, None, P, P, big, *g3, 1, None) == -1 and err() == "u, v or w pointer not aligned to its element type"
    for q in range(3, 6):
        a = list(six)
        a[q] = None
        assert tau(*a, None, P, P, big, *g3, 1, None) == -1 and err() == "null dx_fc, dy_cf or dz_f"
        a = list(six)
        a[q] = P + 2
        assert tau(*a, None, P, P, big, *g3, 0, None) == -1 and err() == "dx_fc, dy_cf or dz_f pointer not aligned to its element type"
    assert tau(*six, P + 2, P, P, big, *g3, 1, None) == -1 and err() == "count plane pointer not aligned to int32"
    assert tau(*six, None, None, P, big, *g3, 1, None) == -1 and err() == "null out"
    assert tau(*six, None, P + 4, P, big, *g3, 1, None) == -1 and err() == "out pointer not aligned to double"
    assert tau(*six, None, P, P, big, 2, 65536, 32768, 0, 0, 0, 1, None) == -5 and "32-bit" in err()
    assert tau(*six, None, P, None, big, *g3, 1, None) == -4 and err().startswith("null workspace")
    assert tau(*six, None, P, P + 4, big, *g3, 1, None) == -4 and err() == "workspace not 8-B aligned"
    assert tau(*six, None, P, P, 8, *g3, 1, None) == -4 and err().startswith("workspace too small")


# ---- the time-step wizard ------------------------------------------------------------------------------------------------------------------
def test_wizard_arithmetic(osg):
    wz = osg.TimeStepWizard()
    assert (wz.cfl, wz.max_change, wz.min_change, wz.max_dt, wz.min_dt) == (0.2, 1.1, 0.5, math.inf, 0.0)
    wz = osg.TimeStepWizard(cfl=0.3, max_change=1.1, min_change=0.5)
    assert wz.new_time_step(10.0, 40.0) == min(1.1 * 10.0, 0.3 * 40.0) == 11.0          # cfl * tau = 12: limited by max_change
    assert wz.new_time_step(10.0, 400.0) == 1.1 * 10.0                                  # a tenfold jump in tau: still max_change
    assert wz.new_time_step(10.0, 30.0) == 0.3 * 30.0                                   # inside the band: cfl * tau
    assert wz.new_time_step(10.0, 0.03) == 0.5 * 10.0                                   # a collapse: limited by min_change
    assert wz.new_time_step(10.0, 0.0) == 5.0 and wz.new_time_step(10.0, math.inf) == 11.0
    cl = osg.TimeStepWizard(cfl=0.3, max_dt=10.5, min_dt=6.0)
    assert cl.new_time_step(10.0, 400.0) == 10.5 and cl.new_time_step(10.0, 0.03) == 6.0 and cl.new_time_step(10.0, 30.0) == 9.0
    assert cl.new_time_step(100.0, 1e9) == 10.5 and cl.new_time_step(1.0, 1e-9) == 6.0
    assert math.isnan(wz.new_time_step(10.0, math.nan))
    assert "cfl=0.3" in repr(wz)


# ---- the z face spacings -------------------------------------------------------------------------------------------------------------------
def _host_grid(osg, Nz, z, dtype):
    """an OrthogonalSphericalShellGrid record with host tensors: enough for the host rules that touch no device"""
    import torch
    return osg.OrthogonalSphericalShellGrid(
        architecture=None, Nx=8, Ny=6, Nz=Nz, Hx=1, Hy=1, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10)},
        z_faces=torch.zeros(Nz + 3), z_centers=torch.zeros(Nz + 2), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
        topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=dtype, z_spec=z)


def test_z_face_spacings_host_rule(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd.grids import boundary_z_spacings
    for dtype, npt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        g = _host_grid(osg, 7, (-1, 0), dtype)                     # a regular interval: (z1 - z0) / Nz at every face, rounded once
        d = osg.z_face_spacings(g)
        assert d.dtype == torch.float64 and d.shape == (7,)
        assert np.array_equal(d.numpy(), np.full(7, np.float64(npt(1.0 / 7))))
        assert d[0].item() == boundary_z_spacings(g)[0]
        faces = [-10.0, -6.0, -3.5, -1.7, -0.6, 0.0]               # explicit stretched faces
        g = _host_grid(osg, 5, faces, dtype)
        d = osg.z_face_spacings(g)
        f = np.array(faces)
        c = np.concatenate([[f[0] - (f[1] - f[0]) / 2], (f[1:] + f[:-1]) / 2])      # the halo centre below face 1, then the Nz centres
        assert np.allclose(d.numpy(), np.diff(c), rtol=1e-6 if npt == np.float32 else 1e-15)
        want = np.float64(npt(np.diff(0.5 * (np.concatenate([[f[0] - (f[1] - f[0])], f])[1:] + np.concatenate([[f[0] - (f[1] - f[0])], f])[:-1]))))
        assert np.array_equal(d.numpy(), want)                    # float64 differences of float64 centres, rounded once
        assert d[0].item() == boundary_z_spacings(g)[0]
        assert osg.z_face_spacings(g, torch.float64)[0].item() == boundary_z_spacings(g, torch.float64)[0]
