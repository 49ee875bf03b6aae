"""Host-side tests of w from continuity and the horizontal divergence (no GPU): the export list of libtripolar_hip_continuity.so, every
argument error of tpg_w_from_continuity (status and message; every call below fails in validation, none reaches a launch, the pointers are
never dereferenced), the argument checks of the Python layer and z_center_spacings."""

import pytest


def test_argument_errors_without_device_work(osg):
    from test_abi import declared_symbols, exported_symbols
    lib = osg._lib.continuity_lib()
    # header = exports = signatures
    names = declared_symbols("tripolar_hip_continuity.h")
    assert names == ["tpg_continuity_last_error", "tpg_w_from_continuity"] == exported_symbols(osg._lib.CONTINUITY_LIB_PATH) == sorted(osg._lib.CONTINUITY_SIGNATURES)
    err = lambda: lib.tpg_continuity_last_error().decode()
    call = lambda *a: lib.tpg_w_from_continuity(*a)
    g = (48, 40, 3, 4, 4, 4)
    plane = 56 * 48 * 8
    bytes64, wbytes64 = plane * 11, plane * 12                     # a Float64 parent of u, v, div (Nz + 2Hz planes) and of w (one more)
    base = 1 << 30
    U, V, W, D = base, base + bytes64, base + 2 * bytes64, base + 2 * bytes64 + wbytes64
    DY, DX, AZ, DZ, N = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20
    eight = (U, V, W, D, DY, DX, AZ, DZ)
    assert call(*eight, None, 0.0, *g, 7, None) == -1 and err() == "unknown element type ft=7"
    assert call(*eight, None, 0.0, 49, 40, 3, 4, 4, 4, 1, None) == -2
    for q in (0, 1):
        a = list(eight)
        a[q] = None
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "null u or v"
    a = list(eight)
    a[2] = a[3] = None
    assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "w and div both null: nothing to compute"
    for q in range(4, 8):
        a = list(eight)
        a[q] = None
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "null dy_fc, dx_cf, az_cc or dz_c"
        a = list(eight)
        a[q] = eight[q] + 4
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "dy_fc, dx_cf, az_cc or dz_c pointer not aligned to its element type"
    for q in range(4):
        a = list(eight)
        a[q] = eight[q] + 4
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "u, v, w or div pointer not aligned to its element type"
        a[q] = eight[q] + 2
        assert call(*a, None, 0.0, *g, 0, None) == -1 and err() == "u, v, w or div pointer not aligned to its element type"
    assert call(*eight, N + 2, 0.0, *g, 1, None) == -1 and err() == "count plane pointer not aligned to int32"
    # w's parent (Nz + 1 + 2Hz planes) against u's and v's: identical, one element inside from either side, down to the last element of each
    far = 1 << 36
    for other in (0, 1):
        for shift in (0, 8, -8, bytes64 - 8, 8 - wbytes64):
            a = list(eight)
            a[2], a[3] = eight[other] + shift, far
            a[1 - other] = far + (1 << 32)
            assert call(*a, None, 0.0, *g, 1, None) == -1 and err().startswith("w's parent overlaps u's or v's"), (other, shift)
        # exact: with Hy = 0 the planes are 56 x 40; w right behind u / v, or ending right in front of it, is no overlap (the call goes on
        # to refuse Hy = 0), one element nearer is
        ub0, wb0 = 56 * 40 * 8 * 11, 56 * 40 * 8 * 12
        for shift, status in ((ub0, -5), (ub0 - 8, -1), (-wb0, -5), (8 - wb0, -1)):
            a = list(eight)
            a[2], a[3] = eight[other] + shift, None
            a[1 - other] = far + (1 << 32)
            assert call(*a, None, 0.0, 48, 40, 3, 4, 0, 4, 1, None) == status, (other, shift)
            assert err().startswith("w's parent overlaps u's or v's" if status == -1 else "the rule reads")
        # the last plane of w is what makes it longer than u: w ending one plane into u overlaps, as a parent of u's length would not
        a = list(eight)
        a[2], a[3] = eight[other] - wbytes64 + 8, None
        a[1 - other] = far + (1 << 32)
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err().startswith("w's parent overlaps u's or v's")
        for shift in (0, 8, -8, bytes64 - 8, 8 - bytes64):
            a = list(eight)
            a[2], a[3] = None, eight[other] + shift
            assert call(*a, None, 0.0, *g, 1, None) == -1 and err().startswith("div's parent overlaps u's or v's"), (other, shift)
    for shift in (0, 8, wbytes64 - 8, 8 - bytes64):                # div against w's longer parent
        a = list(eight)
        a[3] = W + shift
        a[0], a[1] = far, far
        assert call(*a, None, 0.0, *g, 1, None) == -1 and err() == "w's parent overlaps div's", shift
    # the overlap test is exact (the calls below get past it and are refused for the missing halo)
    a = list(eight)
    a[0] = a[1] = far
    a[2], a[3] = W, W + 56 * 40 * 8 * 12                           # Hy = 0: planes of 56 x 40
    assert call(*a, None, 0.0, 48, 40, 3, 4, 0, 4, 1, None) == -5 and "Hx >= 1 and Hy >= 1" in err()
    a[3] = W + 56 * 40 * 8 * 12 - 8
    assert call(*a, None, 0.0, 48, 40, 3, 4, 0, 4, 1, None) == -1 and err() == "w's parent overlaps div's"
    a[3] = W - 56 * 40 * 8 * 11
    assert call(*a, None, 0.0, 48, 40, 3, 4, 0, 4, 1, None) == -5
    a[3] = W - 56 * 40 * 8 * 11 + 8
    assert call(*a, None, 0.0, 48, 40, 3, 4, 0, 4, 1, None) == -1 and err() == "w's parent overlaps div's"
    # u and v may be one array; the halo the stencil needs
    a = list(eight)
    a[1] = U
    assert call(*a, None, 0.0, 48, 40, 3, 0, 4, 4, 1, None) == -5 and "Hx >= 1 and Hy >= 1" in err()
    assert call(*eight, None, 0.0, 48, 40, 3, 4, 0, 4, 0, None) == -5 and "Hx >= 1 and Hy >= 1" in err()
    assert call(*eight, N, 0.0, 48, 40, 3, 0, 0, 0, 1, None) == -5
    # more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    assert call(1 << 40, 1 << 41, 1 << 42, 1 << 43, DY, DX, AZ, DZ, None, 0.0, 65536, 32768, 1, 1, 1, 0, 0, None) == -5 and "32-bit" in err()


def _host_grid(osg, dtype=None, z=(-1, 0), Nz=3):
    """an OrthogonalSphericalShellGrid record with host tensors: enough for the checks that touch no device"""
    import torch
    dtype = dtype or torch.float64
    return osg.OrthogonalSphericalShellGrid(
        architecture=None, Nx=8, Ny=6, Nz=Nz, Hx=1, Hy=1, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10, dtype=dtype)},
        z_faces=torch.zeros(Nz + 3), z_centers=torch.zeros(Nz + 2), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
        topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=dtype, z_spec=z)


def test_python_argument_checks(osg):
    import torch
    for name in ("compute_w_from_continuity", "horizontal_divergence", "continuity_plan", "ContinuityPlan", "HorizontalDivergenceField",
                 "z_center_spacings"):
        assert hasattr(osg, name), name
    for name in ("continuity_lib", "check_continuity", "CONTINUITY_SIGNATURES", "CONTINUITY_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    grid, other = _host_grid(osg), _host_grid(osg)
    F, Cc = osg.Face, osg.Center
    u, v, c, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid), osg.ZFaceField(grid)
    for call in (lambda a, b: osg.compute_w_from_continuity(a, b), lambda a, b: osg.horizontal_divergence(a, b),
                 lambda a, b: osg.continuity_plan(a, b, w, c), lambda a, b: osg.HorizontalDivergenceField(a, b)):
        with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
            call(v, v)
        with pytest.raises(TypeError, match=r"v must be a Field at \(Center, Face, Center\)"):
            call(u, c)
        with pytest.raises(TypeError, match="u must be a Field"):
            call(u.data, v)
        with pytest.raises(ValueError, match="one grid"):
            call(u, osg.YFaceField(other))
        v32 = osg.YFaceField(grid, data=torch.zeros(v.data.shape, dtype=torch.float32))
        with pytest.raises(ValueError, match="one element type"):
            call(u, v32)
        with pytest.raises(NotImplementedError, match="z-windowed"):
            call(u, osg.YFaceField(grid, indices=(slice(None), slice(None), range(1, 3))))
        with pytest.raises(NotImplementedError, match="z-windowed"):
            call(osg.XFaceField(grid, indices=(slice(None), slice(None), 2)), v)
    # the outputs: at least one; a wrong location is a TypeError naming the output
    with pytest.raises(TypeError, match="at least one output"):
        osg.continuity_plan(u, v)
    with pytest.raises(TypeError, match=r"w must be a Field at \(Center, Center, Face\)"):
        osg.compute_w_from_continuity(u, v, c)
    with pytest.raises(TypeError, match=r"w must be a Field at \(Center, Center, Face\)"):
        osg.continuity_plan(u, v, c, c)
    with pytest.raises(TypeError, match=r"div must be a Field at \(Center, Center, Center\)"):
        osg.horizontal_divergence(u, v, out=w)
    with pytest.raises(TypeError, match=r"div must be a Field at \(Center, Center, Center\)"):
        osg.continuity_plan(u, v, w, w)
    with pytest.raises(ValueError, match="one grid"):
        osg.compute_w_from_continuity(u, v, osg.ZFaceField(other))
    with pytest.raises(ValueError, match="one grid"):
        osg.horizontal_divergence(u, v, out=osg.CenterField(other))
    with pytest.raises(NotImplementedError, match="z-windowed"):
        osg.compute_w_from_continuity(u, v, osg.ZFaceField(grid, indices=(slice(None), slice(None), range(1, 4))))
    with pytest.raises(NotImplementedError, match="z-windowed"):
        osg.horizontal_divergence(u, v, out=osg.CenterField(grid, indices=(slice(None), slice(None), 1)))
    # a reduced field is at no (Face, Center, Center) / (Center, Center, Center)
    with pytest.raises(TypeError, match="u must be a Field at"):
        osg.compute_w_from_continuity(osg.Field((F, Cc, None), grid), v)
    with pytest.raises(TypeError, match="div must be a Field at"):
        osg.horizontal_divergence(u, v, out=osg.Field((Cc, Cc, None), grid))


def test_z_center_spacings_regular_and_explicit_faces(osg):
    import torch
    # a regular interval: (z1 - z0) / Nz at every level, computed in float64 and rounded once
    g = _host_grid(osg, z=(-1, 0), Nz=3)
    d = osg.z_center_spacings(g)
    assert d.dtype == torch.float64 and d.tolist() == [(0.0 - -1.0) / 3] * 3
    d32 = osg.z_center_spacings(g, torch.float32)
    one = torch.tensor(1 / 3, dtype=torch.float64).to(torch.float32).to(torch.float64).item()
    assert d32.dtype == torch.float64 and d32.tolist() == [one] * 3 and one != 1 / 3
    assert osg.z_center_spacings(_host_grid(osg, torch.float32, z=(-1, 0), Nz=3)).tolist() == [one] * 3     # default: the grid's type
    # explicit faces: the float64 differences of adjacent faces, then ONE rounding (not the difference of rounded faces)
    faces = [-1.0, -0.7, -0.1 - 2.0 ** -30, 0.0]
    g = _host_grid(osg, z=faces, Nz=3)
    want = [faces[k + 1] - faces[k] for k in range(3)]
    assert osg.z_center_spacings(g).tolist() == want
    r = lambda x: torch.tensor(x, dtype=torch.float64).to(torch.float32).to(torch.float64).item()
    got32 = osg.z_center_spacings(g, torch.float32).tolist()
    assert got32 == [r(x) for x in want]
    assert got32 != [r(r(faces[k + 1]) - r(faces[k])) for k in range(3)]
    # an ImmersedBoundaryGrid-like wrapper: the underlying grid's
    class Wrapped:
        underlying_grid = g
    assert osg.z_center_spacings(Wrapped()).tolist() == want
