"""Host-side tests of the barotropic mode and the split-explicit velocity correction (no GPU): the export list of
libtripolar_hip_barotropic.so, every argument error of tpg_barotropic_mode and tpg_barotropic_correction (status and message; every call
below fails in validation, none reaches a launch, the pointers are fabricated and never dereferenced), the argument checks of the Python
layer on host-only grid records, and column_depth_table."""

import pytest

NAMES = ["tpg_barotropic_correction", "tpg_barotropic_last_error", "tpg_barotropic_mode"]
G = (48, 40, 3, 4, 4, 4)                                           # Nx, Ny, Nz, Hx, Hy, Hz
HY2 = 13
PARENT = 56 * 48 * 11 * 8                                          # bytes of a Float64 parent of u, v
PLANE = 56 * (40 + 2 * HY2) * 8                                    # bytes of a Float64 2-D plane with Hy2 = 13
FAR = 1 << 36


def test_header_exports_and_signatures_are_the_three_names(osg):
    from test_abi import declared_symbols, exported_symbols
    osg._lib.barotropic_lib()
    assert declared_symbols("tripolar_hip_barotropic.h") == NAMES == exported_symbols(osg._lib.BAROTROPIC_LIB_PATH) == sorted(osg._lib.BAROTROPIC_SIGNATURES)


def test_mode_argument_errors_without_device_work(osg):
    lib = osg._lib.barotropic_lib()
    err = lambda: lib.tpg_barotropic_last_error().decode()
    call = lambda *a: lib.tpg_barotropic_mode(*a)
    base = 1 << 30
    U3, V3, UB, VB, DZ = base, base + PARENT, base + 2 * PARENT, base + 2 * PARENT + PLANE, 1 << 20
    five = (U3, V3, UB, VB, DZ)
    assert call(*five, *G, HY2, 7, None) == -1 and err() == "unknown element type ft=7"
    assert call(*five, 49, 40, 3, 4, 4, 4, HY2, 1, None) == -2
    assert call(*five, *G, -1, 1, None) == -1 and err() == "invalid north/south halo Hy2=-1 of the 2-D planes"
    assert call(None, None, None, None, DZ, *G, HY2, 1, None) == -1 and err() == "u, v, Ubar and Vbar all null: nothing to compute"
    for q, msg in ((0, "u and Ubar"), (2, "u and Ubar"), (1, "v and Vbar"), (3, "v and Vbar")):
        a = list(five)
        a[q] = None
        assert call(*a, *G, HY2, 1, None) == -1 and err() == msg + " must be given together", q
    a = list(five)
    a[4] = None
    assert call(*a, *G, HY2, 1, None) == -1 and err() == "null dz_c"
    for q in range(4):
        a = list(five)
        a[q] = five[q] + 4
        assert call(*a, *G, HY2, 1, None) == -1 and err() == "u, v, Ubar or Vbar pointer not aligned to its element type"
        a[q] = five[q] + 2
        assert call(*a, *G, HY2, 0, None) == -1 and err() == "u, v, Ubar or Vbar pointer not aligned to its element type"
    a = list(five)
    a[4] = DZ + 4
    assert call(*a, *G, HY2, 1, None) == -1 and err() == "dz_c pointer not aligned to its element type"
    # Ubar / Vbar against u's and v's parent: exact to one element on both sides.  A call that gets past every check would launch, so the
    # no-overlap side is shown by the NEXT check refusing: the other plane overlaps the one under test by one element, on its far side
    for out, name in ((2, "Ubar"), (3, "Vbar")):
        for other in (0, 1):
            for shift, overlaps in ((0, True), (8, True), (PARENT - 8, True), (8 - PLANE, True), (PARENT, False), (-PLANE, False)):
                a = [FAR, FAR + (1 << 32), None, None, DZ]
                a[other] = five[other]
                a[out] = five[other] + shift
                a[5 - out] = FAR + (1 << 34) if overlaps else a[out] + (PLANE - 8 if shift > 0 else 8 - PLANE)
                assert call(*a, *G, HY2, 1, None) == -1
                assert err().startswith(f"{name} overlaps u's or v's parent" if overlaps else "Ubar overlaps Vbar"), (name, other, shift, err())
    # Ubar against Vbar: identical, one element inside from either side (the helper is the one held exact on both sides above)
    for shift in (0, 8, PLANE - 8, 8 - PLANE):
        a = [U3, V3, FAR, FAR + shift, DZ]
        assert call(*a, *G, HY2, 1, None) == -1 and err() == "Ubar overlaps Vbar", shift
    # u and v may be one array: the call passes that pair and is refused for the overlap of its outputs
    assert call(U3, U3, FAR, FAR, DZ, *G, HY2, 1, None) == -1 and err() == "Ubar overlaps Vbar"
    # Hy2 = 0 and no halo at all are shapes like any other
    assert call(U3, U3, FAR, FAR, DZ, 48, 40, 3, 0, 0, 0, 0, 1, None) == -1 and err() == "Ubar overlaps Vbar"
    # more work items than 32 bits index: refused by the plane check every entry point shares
    assert call(1 << 40, 1 << 41, 1 << 42, 1 << 43, DZ, 65536, 32768, 1, 1, 1, 0, 0, 0, None) == -5 and "32-bit" in err()


def test_correction_argument_errors_without_device_work(osg):
    lib = osg._lib.barotropic_lib()
    err = lambda: lib.tpg_barotropic_last_error().decode()
    call = lambda *a: lib.tpg_barotropic_correction(*a)
    base = 1 << 30
    U3, V3 = base, base + PARENT
    P = [base + 2 * PARENT + q * PLANE for q in range(4)]          # U, V, Ubar, Vbar
    D, N = 1 << 20, 2 << 20
    seven = (U3, V3, *P, D)
    tail = (None, None, 0.0, *G, HY2, 1, None)
    assert call(*seven, None, None, 0.0, *G, HY2, 7, None) == -1 and err() == "unknown element type ft=7"
    assert call(*seven, None, None, 0.0, *G, -2, 1, None) == -1 and err() == "invalid north/south halo Hy2=-2 of the 2-D planes"
    assert call(None, None, None, None, None, None, D, *tail) == -1 and err() == "u, v, U, V, Ubar and Vbar all null: nothing to compute"
    for q, msg in ((0, "u, U and Ubar"), (2, "u, U and Ubar"), (4, "u, U and Ubar"), (1, "v, V and Vbar"), (3, "v, V and Vbar"), (5, "v, V and Vbar")):
        a = list(seven)
        a[q] = None
        assert call(*a, *tail) == -1 and err() == msg + " must be given together", q
    a = list(seven)
    a[6] = None
    assert call(*a, *tail) == -1 and err() == "null depth_of_count"
    for q in range(6):
        a = list(seven)
        a[q] = seven[q] + 4
        assert call(*a, *tail) == -1 and err() == "u, v, U, V, Ubar or Vbar pointer not aligned to its element type"
        a[q] = seven[q] + 2
        assert call(*a, None, None, 0.0, *G, HY2, 0, None) == -1 and err() == "u, v, U, V, Ubar or Vbar pointer not aligned to its element type"
    a = list(seven)
    a[6] = D + 4
    assert call(*a, *tail) == -1 and err() == "depth_of_count pointer not aligned to its element type"
    for planes in ((N + 2, None), (None, N + 2), (N, N + 1)):
        assert call(*seven, *planes, 0.0, *G, HY2, 1, None) == -1 and err() == "count plane pointer not aligned to int32"
    # each 2-D plane against u's and v's parent, exact to one element on both sides; the no-overlap side is shown by the next check
    # refusing: u == v (both are written)
    names = ("U", "V", "Ubar", "Vbar")
    for q in range(4):
        for shift, overlaps in ((0, True), (8, True), (PARENT - 8, True), (8 - PLANE, True), (PARENT, False), (-PLANE, False)):
            a = [U3, U3, FAR, FAR, FAR, FAR, D]                    # u == v
            a[2 + q] = U3 + shift
            assert call(*a, *tail) == -1
            want = f"{names[q]} overlaps u's or v's parent" if overlaps else "u's parent overlaps v's: both are written"
            assert err().startswith(want), (q, shift, err())
    # u against v, exact: one element inside from either side overlaps
    for shift in (0, 8, PARENT - 8, 8 - PARENT):
        a = [U3, U3 + shift, FAR, FAR, FAR, FAR, D]
        assert call(*a, *tail) == -1 and err() == "u's parent overlaps v's: both are written", shift
    assert call(1 << 40, 1 << 41, 1 << 42, 1 << 43, 1 << 44, 1 << 45, D, None, None, 0.0, 65536, 32768, 1, 1, 1, 0, 0, 0, None) == -5 and "32-bit" in err()


def _host_grid(osg, dtype=None, z=(-1, 0), Nz=3, Hy=1):
    """an OrthogonalSphericalShellGrid record with host tensors: enough for the checks that touch no device"""
    import torch
    dtype = dtype or torch.float64
    return osg.OrthogonalSphericalShellGrid(
        architecture=None, Nx=8, Ny=6, Nz=Nz, Hx=1, Hy=Hy, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(6 + 2 * Hy, 10, dtype=dtype)},
        z_faces=torch.zeros(Nz + 3), z_centers=torch.zeros(Nz + 2), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
        topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=dtype, z_spec=z)


def test_python_argument_checks(osg):
    import torch
    for name in ("compute_barotropic_mode", "barotropic_correction", "barotropic_mode_plan", "BarotropicModePlan", "barotropic_correction_plan",
                 "BarotropicCorrectionPlan", "column_depth_table"):
        assert hasattr(osg, name), name
    for name in ("barotropic_lib", "check_barotropic", "BAROTROPIC_SIGNATURES", "BAROTROPIC_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    grid, other, ext, ext2 = _host_grid(osg), _host_grid(osg), _host_grid(osg, Hy=3), _host_grid(osg, Hy=2)
    F, Cc = osg.Face, osg.Center
    u, v, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    U, V = osg.Field((F, Cc, None), ext), osg.Field((Cc, F, None), ext)
    calls = (lambda a, b: osg.compute_barotropic_mode(a, b), lambda a, b: osg.barotropic_mode_plan(a, b, U, V),
             lambda a, b: osg.barotropic_correction(a, b, U, V), lambda a, b: osg.barotropic_correction_plan(a, b, U, V, U, V))
    for call in calls:
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
    # the 2-D fields: location, shared Nx / Ny / Hx, one Hy2, element type
    for call in (lambda a, b: osg.compute_barotropic_mode(u, v, a, b), lambda a, b: osg.barotropic_mode_plan(u, v, a, b),
                 lambda a, b: osg.barotropic_correction(u, v, a, b), lambda a, b: osg.barotropic_correction_plan(u, v, a, b)):
        with pytest.raises(TypeError, match=r"U must be a Field at \(Face, Center, Nothing\)"):
            call(V, V)
        with pytest.raises(TypeError, match=r"V must be a Field at \(Center, Face, Nothing\)"):
            call(U, u)
        with pytest.raises(TypeError, match="U must be a Field"):
            call(U.data, V)
        with pytest.raises(ValueError, match="one north/south halo"):
            call(U, osg.Field((Cc, F, None), ext2))
        with pytest.raises(ValueError, match="one element type"):
            call(U, osg.Field((Cc, F, None), ext, data=torch.zeros(V.data.shape, dtype=torch.float32)))
        wide = osg.OrthogonalSphericalShellGrid(
            architecture=None, Nx=8, Ny=6, Nz=3, Hx=2, Hy=3, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(12, 12, dtype=torch.float64)},
            z_faces=torch.zeros(6), z_centers=torch.zeros(5), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
            topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=torch.float64, z_spec=(-1, 0))
        with pytest.raises(ValueError, match="must share Nx, Ny and Hx"):
            call(osg.Field((F, Cc, None), wide), osg.Field((Cc, F, None), wide))
    # half-given pairs: in the mode family U without V only with v None; the correction takes all four, and Ubar with Vbar
    for call in (osg.compute_barotropic_mode, osg.barotropic_mode_plan):
        with pytest.raises(TypeError, match="given together"):
            call(u, v, U, None)
        with pytest.raises(TypeError, match="given together"):
            call(u, v, None, V)
        with pytest.raises(TypeError, match="given together"):
            call(u, None, None, V)
        with pytest.raises(TypeError, match="at least one of u"):
            call(None, None)
    for call in (osg.barotropic_correction, osg.barotropic_correction_plan):
        with pytest.raises(TypeError, match="u must be a Field"):
            call(None, v, U, V)
        with pytest.raises(TypeError, match="V must be a Field"):
            call(u, v, U, None)
        with pytest.raises(TypeError, match="Ubar and Vbar are given together"):
            call(u, v, U, V, U, None)
        with pytest.raises(TypeError, match=r"Ubar must be a Field at \(Face, Center, Nothing\)"):
            call(u, v, U, V, V, V)


def test_column_depth_table_regular_and_explicit_faces(osg):
    import torch
    r = lambda x: torch.tensor(x, dtype=torch.float64).to(torch.float32).to(torch.float64).item()
    # a regular interval: faces z0 + (z1 - z0) n / Nz in float64, the last one z1; depth[n] = z1 - face[n], rounded once
    g = _host_grid(osg, z=(-1, 0), Nz=3)
    d = osg.column_depth_table(g)
    want = [0.0 - (-1.0 + 1.0 * n / 3) for n in range(3)] + [0.0]
    assert d.dtype == torch.float64 and d.tolist() == want and d[0].item() == 1.0
    assert d[3].item() == 0 and not torch.signbit(d[3]).item()     # +0
    d32 = osg.column_depth_table(g, torch.float32)
    assert d32.dtype == torch.float64 and d32.tolist() == [r(x) for x in want] and d32.tolist() != want
    assert d32[3].item() == 0 and not torch.signbit(d32[3]).item()
    assert osg.column_depth_table(_host_grid(osg, torch.float32, z=(-1, 0), Nz=3)).tolist() == d32.tolist()     # default: the grid's type
    g = _host_grid(osg, z=(-4000.1, 0.3), Nz=3)
    assert osg.column_depth_table(g)[0].item() == 0.3 - -4000.1 and osg.column_depth_table(g, torch.float32)[0].item() == r(0.3 - -4000.1)
    # explicit faces: the float64 differences from the top face, then ONE rounding (not the difference of rounded faces)
    faces = [-1.0, -0.7, 3 * 2.0 ** -28, 0.25 + 2.0 ** -27]
    g = _host_grid(osg, z=faces, Nz=3)
    want = [faces[3] - faces[n] for n in range(4)]
    assert osg.column_depth_table(g).tolist() == want and want[3] == 0 and want[0] == 1.25 + 2.0 ** -27
    got32 = osg.column_depth_table(g, torch.float32)
    assert got32.tolist() == [r(x) for x in want] and got32.tolist() != [r(r(faces[3]) - r(faces[n])) for n in range(4)]
    assert got32[3].item() == 0 and not torch.signbit(got32[3]).item()
    # an ImmersedBoundaryGrid-like wrapper: the underlying grid's
    class Wrapped:
        underlying_grid = g
    assert osg.column_depth_table(Wrapped()).tolist() == want
