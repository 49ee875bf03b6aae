"""Host-side tests of the vertical vorticity (no GPU): every argument error of tpg_vertical_vorticity (status and message; every call below
fails in validation, none reaches a launch, the pointers are never dereferenced) and the argument checks of the Python layer."""

import pytest


def test_argument_errors_without_device_work(osg):
    from test_abi import declared_symbols, exported_symbols
    lib = osg._lib.operators_lib()
    # header = exports = signatures, for the operators library as for the product's; the test build adds the knob reload and nothing else
    names = declared_symbols("tripolar_hip_operators.h")
    assert names == ["tpg_operators_last_error", "tpg_vertical_vorticity"] == exported_symbols(osg._lib.OPERATORS_LIB_PATH) == sorted(osg._lib.OPERATORS_SIGNATURES)
    from tools import testlib
    assert exported_symbols(testlib.OPERATORS_LIB_PATH) == sorted(names + ["tpg_reload_config"])
    assert "tpg_vertical_vorticity" not in exported_symbols(osg._lib.LIB_PATH) and osg._lib.lib().tpg_version() == 600
    err = lambda: lib.tpg_operators_last_error().decode()
    call = lambda *a: lib.tpg_vertical_vorticity(*a)
    g = (48, 40, 3, 4, 4, 4)
    bytes64 = 56 * 48 * 11 * 8                                     # one Float64 parent of that geometry
    U, V, Z, DX, DY, AZ, N = (1 << 30) + 0 * bytes64, (1 << 30) + 1 * bytes64, (1 << 30) + 2 * bytes64, 1 << 20, 2 << 20, 3 << 20, 4 << 20
    six = (U, V, Z, DX, DY, AZ)
    assert call(*six, None, 0.0, *g, 7, None) == -1 and err() == "unknown element type ft=7"
    assert call(*six, None, 0.0, 49, 40, 3, 4, 4, 4, 1, None) == -2
    for q in range(3):
        a = list(six)
        a[q] = None
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "null u, v or zeta"
        a = list(six)
        a[q] = six[q] + 4
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "u, v or zeta pointer not aligned to its element type"
        a[q] = six[q] + 2
        assert call(*a, None, 0.0, *g, 0, None) == -1 and err() == "u, v or zeta pointer not aligned to its element type"
    for q in range(3, 6):
        a = list(six)
        a[q] = None
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "null dx_fc, dy_cf or az_ff"
        a = list(six)
        a[q] = six[q] + 4
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "dx_fc, dy_cf or az_ff pointer not aligned to its element type"
    assert call(*six, N + 2, 0.0, *g, 1, None) == -1 and err() == "count plane pointer not aligned to int32"
    # zeta's parent against u's and v's: identical, one element inside from either side, down to the last element
    for other in (0, 1):
        for shift in (0, 8, -8, bytes64 - 8, 8 - bytes64):
            a = list(six)
            a[2] = six[other] + shift
            assert call(*a, None, 0.0, *g, 1, None) == -1 and err().startswith("zeta's parent overlaps u's or v's"), (other, shift)
    # the halo the stencil needs (Float32 parents, and parents without an x halo, are shorter: the same addresses do not overlap)
    assert call(*six, None, 0.0, 48, 40, 3, 0, 4, 4, 1, None) == -5 and "Hx >= 1 and Hy >= 1" in err()
    assert call(*six, None, 0.0, 48, 40, 3, 4, 0, 4, 0, None) == -5 and "Hx >= 1 and Hy >= 1" in err()
    assert call(*six, N, 0.0, 48, 40, 3, 0, 0, 0, 1, None) == -5
    # the overlap test is exact: with Hx = 0 a parent is 48 * 48 * 11 doubles; zeta right behind u is no overlap (the call goes on to refuse
    # Hx = 0), one element earlier is
    bytes0 = 48 * 48 * 11 * 8
    assert call(U, 1 << 34, U + bytes0, DX, DY, AZ, None, 0.0, 48, 40, 3, 0, 4, 4, 1, None) == -5
    assert call(U, 1 << 34, U + bytes0 - 8, DX, DY, AZ, None, 0.0, 48, 40, 3, 0, 4, 4, 1, None) == -1 and err().startswith("zeta's parent overlaps")
    assert call(U + bytes0, 1 << 34, U, DX, DY, AZ, None, 0.0, 48, 40, 3, 0, 4, 4, 1, None) == -5
    assert call(1 << 34, U + bytes0 - 8, U, DX, DY, AZ, None, 0.0, 48, 40, 3, 0, 4, 4, 1, None) == -1 and err().startswith("zeta's parent overlaps")
    # more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    assert call(1 << 40, 1 << 41, 1 << 42, DX, DY, AZ, None, 0.0, 65536, 32768, 1, 1, 1, 0, 0, None) == -5 and "32-bit" in err()


def _host_grid(osg, dtype=None):
    """an OrthogonalSphericalShellGrid record with host tensors: enough for the checks that touch no device"""
    import torch
    dtype = dtype or torch.float64
    return osg.OrthogonalSphericalShellGrid(
        architecture=None, Nx=8, Ny=6, Nz=3, Hx=1, Hy=1, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10, dtype=dtype)},
        z_faces=torch.zeros(6), z_centers=torch.zeros(5), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
        topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=dtype, z_spec=(-1, 0))


def test_python_argument_checks(osg):
    import torch
    for name in ("vertical_vorticity", "vorticity_plan", "VorticityPlan", "VerticalVorticityField", "compute_"):
        assert hasattr(osg, name), name
    grid, other = _host_grid(osg), _host_grid(osg)
    F, Cc = osg.Face, osg.Center
    u, v, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    zeta = osg.Field((F, F, Cc), grid)
    for call in (lambda a, b: osg.vertical_vorticity(a, b), lambda a, b: osg.vorticity_plan(a, b, zeta),
                 lambda a, b: osg.VerticalVorticityField(a, b)):
        # wrong location
        with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
            call(v, v)
        with pytest.raises(TypeError, match=r"v must be a Field at \(Center, Face, Center\)"):
            call(u, c)
        with pytest.raises(TypeError, match="u must be a Field"):
            call(u.data, v)
        # two grids
        with pytest.raises(ValueError, match="one grid"):
            call(u, osg.YFaceField(other))
        # mixed element type
        v32 = osg.YFaceField(grid, data=torch.zeros(v.data.shape, dtype=torch.float32))
        with pytest.raises(ValueError, match="one element type"):
            call(u, v32)
        # z-windowed
        with pytest.raises(NotImplementedError, match="z-windowed"):
            call(u, osg.YFaceField(grid, indices=(slice(None), slice(None), range(1, 3))))
        with pytest.raises(NotImplementedError, match="z-windowed"):
            call(osg.XFaceField(grid, indices=(slice(None), slice(None), 2)), v)
    # the output field
    with pytest.raises(TypeError, match=r"zeta must be a Field at \(Face, Face, Center\)"):
        osg.vertical_vorticity(u, v, out=c)
    with pytest.raises(TypeError, match="zeta must be a Field"):
        osg.vorticity_plan(u, v, None)
    with pytest.raises(ValueError, match="one grid"):
        osg.vertical_vorticity(u, v, out=osg.Field((F, F, Cc), other))
    with pytest.raises(NotImplementedError, match="z-windowed"):
        osg.vertical_vorticity(u, v, out=osg.Field((F, F, Cc), grid, indices=(slice(None), slice(None), 1)))
    # a reduced field is at no (Face, Center, Center)
    with pytest.raises(TypeError, match="u must be a Field at"):
        osg.vertical_vorticity(osg.Field((F, Cc, None), grid), v)
    with pytest.raises(TypeError, match="no plan to run"):
        osg.compute_(zeta)
