"""Host-side tests of the grid-fitted immersed boundary (no GPU): the numpy reference of tests/immersed_ref.py on hand-made columns, the
count-plane shortcut against the predicate, the two C symbols (declared, exported, bound), every argument error of
tpg_immersed_column_counts / tpg_mask_immersed_fields (status and message, no device work), and the argument validation of
GridFittedBottom / ImmersedBoundaryGrid that precedes device work."""
import ctypes as C
import os

import numpy as np
import pytest

from immersed_ref import chunk_classes, column_counts, draw_columns, heights_of, inactive_cells, mask_immersed_field, peripheral

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.0


def _flat(Nx, Ny, Hx, Hy, dtype, value):
    return np.full((Ny + 2 * Hy, Nx + 2 * Hx), value, dtype=dtype)


def _zc(Nz, dtype):
    return ((np.arange(Nz) + 0.5) / Nz).astype(dtype)             # z = (0, 1)


def _masked(loc, h, zc, size, halo, wall=True):
    Nx, Ny, Nz = size
    Hx, Hy, Hz = halo
    parent = np.full((Nz + loc[2] + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), SENTINEL, dtype=h.dtype)
    out, per = mask_immersed_field(parent, loc, 0.0, h, zc, size, halo, wall)
    inner = out[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert np.array_equal(inner == 0, per)
    touched = out != SENTINEL
    touched[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
    assert not touched.any()                                       # no halo cell, and not level Nz + 1 of a z-Face field
    return per


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_x_face_node_is_masked_iff_either_neighbour_is(dtype):
    size, halo = (8, 6, 2), (2, 2, 1)
    Nx, Ny, Nz = size
    zc = _zc(Nz, dtype)
    h = _flat(Nx, Ny, 2, 2, dtype, -1)
    h[2 + 3, 2 + 4] = 0.3                                          # cell i = 5, j = 4: level 1 (centre 0.25) immersed, level 2 (0.75) not
    pc = _masked((0, 0, 0), h, zc, size, halo)
    pu = _masked((1, 0, 0), h, zc, size, halo)
    assert pc.sum() == 1 and pc[0, 3, 4]
    assert pu.sum() == 2 and pu[0, 3, 4] and pu[0, 3, 5]           # faces i = 5 and i = 6 of row 4
    pv = _masked((0, 1, 0), h, zc, size, halo)
    assert pv[:, 1:].sum() == 2 and pv[0, 3, 4] and pv[0, 4, 4]    # beside the wall row
    pz = _masked((1, 1, 0), h, zc, size, halo)
    assert pz[:, 1:].sum() == 4


def test_i_equal_1_reads_cell_nx_through_the_halo_column():
    size, halo = (8, 4, 1), (1, 1, 0)
    zc = _zc(1, np.float64)
    h = _flat(8, 4, 1, 1, np.float64, -1)
    h[1 + 1, 0] = 1.0                                              # the WEST HALO cell (i = 0) of row j = 2 is land; interior cell Nx is not
    pu = _masked((1, 0, 0), h, zc, size, halo)
    assert pu.sum() == 1 and pu[0, 1, 0]
    assert not _masked((0, 0, 0), h, zc, size, halo).any()
    n = column_counts(h, zc, size, halo, True)
    assert n["fc"][1, 0] == 1 and n["fc"].sum() == 1 and n["cc"].sum() == 0


def test_j_equal_1_of_a_y_face_field_on_a_wall_and_on_a_seam():
    size, halo = (6, 4, 3), (1, 1, 1)
    zc = _zc(3, np.float64)
    h = _flat(6, 4, 1, 1, np.float64, -1)
    h[0, 1 + 2] = 0.6                                              # seam halo row j = 0, cell i = 3: two levels immersed
    wall = _masked((0, 1, 0), h, zc, size, halo, wall=True)
    assert wall[:, 0].all() and not wall[:, 1:].any()              # behind the wall every level of row 1 is peripheral
    seam = _masked((0, 1, 0), h, zc, size, halo, wall=False)
    assert seam.sum() == 2 and seam[0, 0, 2] and seam[1, 0, 2]
    n = column_counts(h, zc, size, halo, False)
    assert n["cf"][0, 2] == 2 and n["cf"].sum() == 2 and n["ff"][0, 2] == 2 and n["ff"][0, 3] == 2 and n["ff"].sum() == 4
    assert (column_counts(h, zc, size, halo, True)["cf"][0] == 3).all()
    assert not _masked((0, 0, 0), h, zc, size, halo, wall=True).any()      # a Center row is not touched by the wall


def test_z_face_field_is_masked_up_to_min_n_plus_1_nz():
    size, halo = (4, 3, 3), (1, 1, 2)
    zc = _zc(3, np.float64)
    h = _flat(4, 3, 1, 1, np.float64, -1)
    h[1, 1:5] = [-1, 0.2, 0.6, 2.0]                                # row 1: counts 0, 1, 2, 3
    pw = _masked((0, 0, 1), h, zc, size, halo)
    assert [int(pw[:, 0, i].sum()) for i in range(4)] == [1, 2, 3, 3]
    assert pw[0].all()                                             # face k = 1 touches cell k = 0 everywhere
    n = column_counts(h, zc, size, halo, True)["cc"]
    assert list(n[0]) == [0, 1, 2, 3]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_height_equal_to_a_centre_is_immersed(dtype):
    size, halo = (4, 2, 3), (1, 1, 1)
    zc = _zc(3, dtype)
    h = _flat(4, 2, 1, 1, dtype, -1)
    h[1, 1] = zc[1]                                                # exactly the second centre, in the grid's type
    h[1, 2] = np.nextafter(zc[1], dtype(-1))                       # one ulp below it
    n = column_counts(h, zc, size, halo, True)["cc"]
    assert n[0, 0] == 2 and n[0, 1] == 1
    pc = _masked((0, 0, 0), h, zc, size, halo)
    assert pc[:, 0, 0].tolist() == [True, True, False] and pc[:, 0, 1].tolist() == [True, False, False]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("wall", [True, False])
def test_count_planes_describe_the_predicate(dtype, wall):
    """the consequence the kernels use: per location, a z-Center field is peripheral for k <= n, a z-Face field for k <= min(n + 1, Nz)"""
    rng = np.random.default_rng(5)
    for size, halo in (((12, 10, 4), (2, 3, 1)), ((48, 40, 3), (4, 4, 4)), ((50, 40, 6), (5, 5, 5))):
        Nx, Ny, Nz = size
        zc = _zc(Nz, dtype)
        h = rng.uniform(-0.2, 1.2, (Ny + 2 * halo[1], Nx + 2 * halo[0])).astype(dtype)
        h[rng.random(h.shape) < 0.3] = zc[rng.integers(0, Nz)]
        n = column_counts(h, zc, size, halo, wall)
        ina = inactive_cells(h, zc, size, halo, wall)
        k = np.arange(1, Nz + 1)[:, None, None]
        for xl in (0, 1):
            for yl in (0, 1):
                plane = n["cf"[xl] + "cf"[yl]]
                assert np.array_equal(peripheral(ina, (xl, yl, 0), size), k <= plane[None])
                assert np.array_equal(peripheral(ina, (xl, yl, 1), size), k <= np.minimum(plane + 1, Nz)[None])


@pytest.mark.parametrize("size", [(48, 40, 3), (48, 40, 6), (50, 40, 3)])
def test_drawn_columns_hold_every_chunk_class_at_every_level(size):
    Nx, Ny, Nz = size
    for dtype in (np.float32, np.float64):
        rng = np.random.default_rng(1234)
        zc = _zc(Nz, dtype)
        c = draw_columns(rng, Nx, Ny, Nz)
        h = heights_of(c, zc, rng)
        assert (h == zc[np.maximum(c, 1) - 1]).any()               # some heights sit exactly on a centre
        for W in (2, 4):
            assert all(all(t) for t in chunk_classes(c, Nz, W)), (size, W)


def test_the_fill_never_unmasks_on_the_host(oracle):
    """mask(fill(mask(f))) == fill(mask(f)) on the interior for c and u with value 0, compared as numbers: the filled bottom's row Ny is
    mirror-symmetric, so an x-Face node (i, Ny), i > Nx/2, and its fold source touch mirrored pairs of cells"""
    size, halo = (12, 10, 4), (3, 3, 2)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(77)
    zc = _zc(Nz, np.float64)
    for _ in range(40):
        h = np.zeros((1, Ny + 2 * Hy, Nx + 2 * Hx))
        h[0, Hy:Hy + Ny, Hx:Hx + Nx] = heights_of(rng.integers(0, Nz + 1, (Ny, Nx)), zc, rng)
        oracle.fill_halo_regions(h, 0, 0, 1, (Nx, Ny, 1), (Hx, Hy, 0))
        row = h[0, Hy + Ny - 1, Hx:Hx + Nx]
        assert np.array_equal(row, row[::-1])
        for loc, sg in (((0, 0, 0), 1), ((1, 0, 0), -1)):
            f = rng.uniform(-1, 1, (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx))
            m1, per = mask_immersed_field(f, loc, 0.0, h[0], zc, size, halo)
            oracle.fill_halo_regions(m1, loc[0], loc[1], sg, size, halo)
            m2, _ = mask_immersed_field(m1, loc, 0.0, h[0], zc, size, halo)
            assert (m1 == m2).all(), loc


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
NAMES = ["tpg_immersed_column_counts", "tpg_mask_immersed_fields"]


def test_both_symbols_are_declared_exported_and_bound(osg):
    from test_abi import declared_symbols, exported_symbols
    lib = osg._lib.lib()
    for n in NAMES:
        assert n in declared_symbols() and n in exported_symbols(osg._lib.LIB_PATH) and n in osg._lib.SIGNATURES and hasattr(lib, n)
    assert lib.tpg_version() == 600
    for name in ("GridFittedBottom", "ImmersedBoundaryGrid", "immersed_mask_plan", "mask_immersed_field"):
        assert hasattr(osg, name)


def test_argument_errors_without_device_work(osg):
    lib = osg._lib.lib()
    P = 1 << 20                                                    # a non-NULL pointer that is never dereferenced
    err = lambda: lib.tpg_last_error().decode()
    g2 = (48, 40, 3, 4, 4)
    cnt = lambda *a: lib.tpg_immersed_column_counts(*a)
    assert cnt(P, P, 1, P, P, P, P, *g2, 7, None) == -1 and err() == "unknown element type ft=7"
    assert cnt(P, P, 1, P, P, P, P, 49, 40, 3, 4, 4, 1, None) == -2
    assert cnt(None, P, 1, P, P, P, P, *g2, 1, None) == -1 and err() == "null bottom_height or z_centers"
    assert cnt(P, None, 1, P, P, P, P, *g2, 1, None) == -1 and err() == "null bottom_height or z_centers"
    assert cnt(P + 4, P, 1, P, P, P, P, *g2, 1, None) == -1 and "not aligned to its element type" in err()
    assert cnt(P, P + 4, 1, P, P, P, P, *g2, 1, None) == -1 and "not aligned to its element type" in err()
    assert cnt(P + 2, P, 1, P, P, P, P, *g2, 0, None) == -1 and "not aligned to its element type" in err()
    assert cnt(P, P, 1, P, P + 2, P, P, *g2, 1, None) == -1 and err() == "count plane pointer not aligned to int32"
    assert cnt(P, P, 1, P, P, None, None, 48, 40, 3, 0, 4, 1, None) == -5 and "Hx >= 1" in err()
    assert cnt(P, P, 1, None, None, None, P, 48, 40, 3, 0, 4, 1, None) == -5 and "Hx >= 1" in err()
    assert cnt(P, P, 0, None, None, P, None, 48, 40, 3, 4, 0, 1, None) == -5 and "Hy >= 1" in err()
    assert cnt(P, P, 0, None, None, None, P, 48, 40, 3, 4, 0, 1, None) == -5 and "Hy >= 1" in err()
    assert cnt(P, P, 1, P, P, P, P, 65536, 32768, 3, 4, 4, 1, None) == -5
    assert cnt(P, P, 1, None, None, None, None, *g2, 1, None) == 0            # nothing asked for: no launch

    good, null_field = (C.c_void_p * 1)(P), (C.c_void_p * 1)(None)
    planes, null_plane = (C.c_void_p * 1)(P), (C.c_void_p * 1)(None)
    zl, vals = (C.c_int8 * 1)(0), (C.c_double * 1)(0.0)
    g3 = (48, 40, 3, 4, 4, 4)
    msk = lambda *a: lib.tpg_mask_immersed_fields(*a)
    assert msk(good, 1, planes, zl, vals, *g3, 7, None) == -1 and err() == "unknown element type ft=7"
    assert msk(good, 1, planes, zl, vals, 49, 40, 3, 4, 4, 4, 1, None) == -2
    assert msk(good, 0, planes, zl, vals, *g3, 1, None) == -1 and err() == "no fields"
    assert msk(None, 1, planes, zl, vals, *g3, 1, None) == -1 and err() == "no fields"
    assert msk(null_field, 1, planes, zl, vals, *g3, 1, None) == -1 and err() == "null field 0"
    for tables in ((None, zl, vals), (planes, None, vals), (planes, zl, None)):
        assert msk(good, 1, *tables, *g3, 1, None) == -1 and err() == "null counts, zloc or values table"
    assert msk(good, 1, null_plane, zl, vals, *g3, 1, None) == -1 and err() == "field 0: null count plane"
    for bad in (2, -1):
        assert msk(good, 1, planes, (C.c_int8 * 1)(bad), vals, *g3, 1, None) == -1 and "neither TPG_CENTER nor TPG_FACE" in err()
    assert msk((C.c_void_p * 1)(P + 4), 1, planes, zl, vals, *g3, 1, None) == -1 and err() == "field 0: pointer not aligned to its element type"
    assert msk((C.c_void_p * 1)(P + 2), 1, planes, zl, vals, *g3, 0, None) == -1 and err() == "field 0: pointer not aligned to its element type"
    assert msk(good, 1, (C.c_void_p * 1)(P + 2), zl, vals, *g3, 1, None) == -1 and err() == "field 0: count plane pointer not aligned to int32"
    assert msk(good, 1, planes, zl, vals, 65536, 32768, 3, 4, 4, 4, 1, None) == -5
    # a fault in the SECOND batch of a table is found before the first batch is launched
    n = 17
    many = (C.c_void_p * n)(*([P] * n))
    zbad = (C.c_int8 * n)(*([0] * 16 + [5]))
    assert msk(many, n, many, zbad, (C.c_double * n)(), *g3, 1, None) == -1 and err().startswith("field 16: zloc = 5")


# ---- the Python host: validation that precedes device work ----------------------------------------------------------------------------
def _host_grid(osg, z_centers):
    """an OrthogonalSphericalShellGrid record with host tensors: enough for the checks that run before any device work"""
    import torch
    Nz = len(z_centers)
    return osg.OrthogonalSphericalShellGrid(
        architecture=None, Nx=8, Ny=6, Nz=Nz, Hx=1, Hy=1, Hz=0, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10)},
        z_faces=torch.zeros(Nz + 1), z_centers=torch.tensor(z_centers, dtype=torch.float64), radius=1.0,
        conformal_mapping=osg.Tripolar(55, 70, -80), topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded))


def test_grid_fitted_bottom_and_immersed_grid_validation(osg):
    for bad in ("deep", None, True, [1, 2]):
        with pytest.raises(TypeError, match="GridFittedBottom"):
            osg.GridFittedBottom(bad)
    for ok in (0, -1.5, np.zeros((6, 8)), lambda lam, phi: 0.0):
        osg.GridFittedBottom(ok)
    ib = osg.GridFittedBottom(0.0)
    with pytest.raises(TypeError, match="TripolarGrid"):
        osg.ImmersedBoundaryGrid(object(), ib)
    grid = _host_grid(osg, [0.25, 0.75])
    with pytest.raises(TypeError, match="GridFittedBottom"):
        osg.ImmersedBoundaryGrid(grid, 0.0)
    for zc in ([0.75, 0.25], [0.25, 0.25, 0.75]):
        with pytest.raises(ValueError, match="strictly increasing"):
            osg.ImmersedBoundaryGrid(_host_grid(osg, zc), ib)

    class Wrapped:                                                 # an immersed grid cannot be wrapped again, nor re-haloed
        underlying_grid = grid

    with pytest.raises(TypeError, match="bare"):
        osg.ImmersedBoundaryGrid(Wrapped(), ib)
    with pytest.raises(NotImplementedError, match="with_halo of an ImmersedBoundaryGrid"):
        osg.with_halo((5, 5, 5), Wrapped())
