"""Host-side tests of the split-explicit free-surface sub-step (no GPU): the export list of libtripolar_hip_free_surface.so, every argument
error of tpg_free_surface_substep (status and message; every call below fails in validation, none reaches a launch, the pointers are
fabricated and never dereferenced), every refusal of the Python layer on host-only grid records, and the ping-pong bookkeeping of the
sub-cycle for odd and even sub-step counts."""

import pytest

from test_barotropic_conditions import _host_grid

NAMES = ["tpg_free_surface_last_error", "tpg_free_surface_substep"]
NX, NY, NZ, HX, HY2 = 48, 40, 3, 4, 13
PLANE = (NX + 2 * HX) * (NY + 2 * HY2) * 8                          # bytes of a Float64 plane
ARGS = ("eta_out", "U_out", "V_out", "eta_in", "U_in", "V_in", "GU", "GV", "eta_bar", "U_bar", "V_bar", "dy_fc", "dx_cf", "az_cc", "dx_fc",
        "dy_cf", "depth_of_count", "n_fc", "n_cf")
BASE = 1 << 30
FAR = 1 << 40


def _pointers():
    """19 fabricated pointers: 16 disjoint planes, the depth table, two count planes"""
    p = {name: BASE + q * PLANE for q, name in enumerate(ARGS[:16])}
    p.update(depth_of_count=1 << 20, n_fc=2 << 20, n_cf=3 << 20)
    return p


def _call(lib, p, geom=(NX, NY, NZ, HX, HY2), ft=1):
    return lib.tpg_free_surface_substep(*(p[k] for k in ARGS), 0.5, 9.8, 0.1, *geom, ft, None)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import declared_symbols, exported_symbols
    osg._lib.free_surface_lib()
    assert declared_symbols("tripolar_hip_free_surface.h") == NAMES == exported_symbols(osg._lib.FREE_SURFACE_LIB_PATH) == sorted(osg._lib.FREE_SURFACE_SIGNATURES)


def test_substep_argument_errors_without_device_work(osg):
    lib = osg._lib.free_surface_lib()
    err = lambda: lib.tpg_free_surface_last_error().decode()
    good = _pointers()
    assert _call(lib, good, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _call(lib, good, (49, NY, NZ, HX, HY2)) == -2
    assert _call(lib, good, (NX, 0, NZ, HX, HY2)) == -1
    for Hx, Hy2 in ((0, HY2), (HX, 0), (-1, HY2), (HX, -3)):
        assert _call(lib, good, (NX, NY, NZ, Hx, Hy2)) == -1 and err().startswith("the rule reads U[i+1, j] and V[i, j+1]: Hx >= 1 and Hy2 >= 1 needed"), (Hx, Hy2)
    for name in ARGS[:8]:
        assert _call(lib, {**good, name: None}) == -1 and err() == "null eta_out, U_out, V_out, eta_in, U_in, V_in, GU or GV", name
    for name in ARGS[11:16]:
        assert _call(lib, {**good, name: None}) == -1 and err() == "null dy_fc, dx_cf, az_cc, dx_fc or dy_cf", name
    assert _call(lib, {**good, "depth_of_count": None}) == -1 and err() == "null depth_of_count"
    # a half-given averaging triple: one missing, two missing
    bars = ARGS[8:11]
    for missing in ([bars[0]], [bars[1]], [bars[2]], bars[:2], bars[1:], [bars[0], bars[2]]):
        assert _call(lib, {**good, **{k: None for k in missing}}) == -1 and err() == "eta_bar, U_bar and V_bar must be given together", missing
    # alignment: every plane and the table to the element, the count planes to int32
    for name in ARGS[:17]:
        assert _call(lib, {**good, name: good[name] + 4}) == -1 and err() == f"{name} pointer not aligned to its element type", name
        assert _call(lib, {**good, name: good[name] + 2}, ft=0) == -1 and err() == f"{name} pointer not aligned to its element type", name
    for name in ARGS[17:]:
        assert _call(lib, {**good, name: good[name] + 2}) == -1 and err() == "count plane pointer not aligned to int32", name
    # every written plane against every other array of the call, exact to one element on both sides.  A call that gets past every check
    # would launch, so the no-overlap side is shown by the LAST check refusing: Ny = 1, with the planes sized for it
    written = ARGS[:3] + ARGS[8:11]
    for out in written:
        for other in ARGS[:16]:
            if other == out:
                continue
            for shift in (0, 8, PLANE - 8, 8 - PLANE):
                p = {**good, other: FAR, out: FAR + shift}
                assert _call(lib, p) == -1 and " overlaps " in err() and out in err() and other in err(), (out, other, shift, err())
    one = (NX + 2 * HX) * (1 + 2 * HY2) * 8                        # a plane with Ny = 1
    for out in written:
        for shift in (one, -one):
            p = {**good, "GU": FAR, out: FAR + shift}
            assert _call(lib, p, (NX, 1, NZ, HX, HY2)) == -5 and err() == "free surface: Ny >= 2 needed (row 1 of V is the wall's)", (out, shift, err())
        assert _call(lib, {**good, "GU": FAR, out: FAR + one - 8}, (NX, 1, NZ, HX, HY2)) == -1 and " overlaps " in err()
    assert _call(lib, {**good, "eta_out": good["eta_in"]}) == -1 and err().startswith("eta_out overlaps eta_in")
    for out in written:
        for k, size in (("depth_of_count", (NZ + 1) * 8), ("n_fc", NX * NY * 4), ("n_cf", NX * NY * 4)):
            for shift in (0, size - 8, 8 - PLANE):
                p = {**good, k: FAR, out: FAR + shift}
                assert _call(lib, p) == -1 and err() == f"{out} overlaps depth_of_count or a count plane", (out, k, shift, err())
    # without the averaging triple and without count planes the same checks hold
    bare = {**good, **{k: None for k in ARGS[8:11] + ARGS[17:]}}
    assert _call(lib, {**bare, "V_out": bare["U_in"] + 8}) == -1 and err().startswith("V_out overlaps U_in")
    assert _call(lib, bare, (NX, 1, NZ, HX, HY2)) == -5
    # more work items than 32 bits index
    huge = {k: (q + 1) << 44 for q, k in enumerate(ARGS)}
    assert _call(lib, huge, (65536, 32768, 1, 1, 1), 0) == -5 and "32-bit" in err()


def test_subcycle_schedule_ends_in_the_callers_fields(osg):
    from orthogonalsphericalshellgrids.jl_amd.free_surface import subcycle_schedule
    for n in range(1, 33):
        copy_first, steps = subcycle_schedule(n)
        assert len(steps) == n and copy_first == (n % 2 == 1)
        held = ["state 0", None]                                   # what each set holds: set 0 is the caller's eta, U, V
        if copy_first:
            held[1] = held[0]
        for s, (src, dst) in enumerate(steps):
            assert {src, dst} == {0, 1}
            assert held[src] == f"state {s}", (n, s)               # every sub-step reads the newest state ...
            held[dst] = f"state {s + 1}"                           # ... and writes the other set
        assert held[0] == f"state {n}"                             # the final state is in the caller's fields
    assert subcycle_schedule(1) == (True, [(1, 0)]) and subcycle_schedule(2) == (False, [(0, 1), (1, 0)])
    assert subcycle_schedule(3) == (True, [(1, 0), (0, 1), (1, 0)])


def test_python_refusals(osg):
    import torch
    for name in ("SplitExplicitFreeSurface", "SplitExplicitSubcyclePlan", "split_explicit_subcycle_plan", "split_explicit_substep"):
        assert hasattr(osg, name), name
    for name in ("free_surface_lib", "check_free_surface", "FREE_SURFACE_SIGNATURES", "FREE_SURFACE_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    grid, other = _host_grid(osg, Hy=3), _host_grid(osg, Hy=3)
    F, Cc = osg.Face, osg.Center
    loc = {"eta": (Cc, Cc, None), "U": (F, Cc, None), "V": (Cc, F, None)}
    new = lambda k, g=grid, **kw: osg.Field(loc[k], g, **kw)
    names = ("eta_out", "U_out", "V_out", "eta", "U", "V", "GU", "GV")
    keys = ("eta", "U", "V", "eta", "U", "V", "U", "V")
    good = [new(k) for k in keys]
    call = lambda a, **kw: osg.split_explicit_substep(*a, 0.5, **kw)
    # wrong locations, and what is no Field
    wrong = {"eta": new("U"), "U": new("V"), "V": new("eta")}
    shown = {"eta": "Center, Center, Nothing", "U": "Face, Center, Nothing", "V": "Center, Face, Nothing"}
    for q, (name, k) in enumerate(zip(names, keys)):
        a = list(good)
        a[q] = wrong[k]
        with pytest.raises(TypeError, match=rf"split_explicit_substep: {name} must be a Field at \({shown[k]}\)"):
            call(a)
        a[q] = good[q].data
        with pytest.raises(TypeError, match=f"{name} must be a Field"):
            call(a)
        a[q] = osg.Field((loc[k][0], loc[k][1], Cc), grid)         # a 3-D field at the same horizontal location
        with pytest.raises(TypeError, match=f"{name} must be a Field"):
            call(a)
        # z-windowed fields
        a[q] = osg.Field((loc[k][0], loc[k][1], Cc), grid, indices=(slice(None), slice(None), 2))
        with pytest.raises(NotImplementedError, match="z-windowed"):
            call(a)
        # different grids, different types
        a[q] = new(k, other)
        with pytest.raises(ValueError, match="one grid"):
            call(a)
        a[q] = new(k, data=torch.zeros(good[q].data.shape, dtype=torch.float32))
        with pytest.raises(ValueError, match="one element type"):
            call(a)
    # the averages: a triple, at the state's locations, of the same grid and type
    with pytest.raises(TypeError, match="given together"):
        call(good, averages=(new("eta"), new("U")))
    with pytest.raises(TypeError, match=r"U_bar must be a Field at \(Face, Center, Nothing\)"):
        call(good, averages=(new("eta"), new("V"), new("V")))
    with pytest.raises(ValueError, match="one grid"):
        call(good, averages=(new("eta"), new("U"), new("V", other)))
    # the grid of the count planes
    with pytest.raises(TypeError, match="grid must be a TripolarGrid"):
        call(good, grid=object())
    with pytest.raises(ValueError, match="must share Nx, Ny and Nz"):
        call(good, grid=_host_grid(osg, Nz=5, Hy=3))
    # a non-tripolar grid, bad sub-step counts, bad weights
    for what in (object(), None, grid.arrays):
        with pytest.raises(TypeError, match="SplitExplicitFreeSurface: grid must be a TripolarGrid"):
            osg.SplitExplicitFreeSurface(what)
    for n in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="substeps must be a positive integer"):
            osg.SplitExplicitFreeSurface(grid, substeps=n)
    with pytest.raises(ValueError, match="weights must be 2 numbers"):
        osg.SplitExplicitFreeSurface(grid, substeps=2, weights=[1.0])
    for what in (None, grid, good[0]):
        with pytest.raises(TypeError, match="free_surface must be a SplitExplicitFreeSurface"):
            osg.split_explicit_subcycle_plan(what, 0.5)
    # a free surface whose extended halo is the grid's own builds on the grid itself: fields, twins, uniform weights
    fs = osg.SplitExplicitFreeSurface(grid, substeps=2)
    assert fs.extended_grid is grid and fs.weights == [0.5, 0.5] and fs.gravitational_acceleration == 9.80665
    assert [f.loc for f in fs.state] == [f.loc for f in fs.twins] == [f.loc for f in fs.averages] == [loc["eta"], loc["U"], loc["V"]]
    assert fs.GU.loc == loc["U"] and fs.GV.loc == loc["V"] and all(f.grid is grid for f in (*fs.state, *fs.twins, *fs.averages, fs.GU, fs.GV))
    assert len({f.data.data_ptr() for f in (*fs.state, *fs.twins, *fs.averages, fs.GU, fs.GV)}) == 11
    assert osg.SplitExplicitFreeSurface(grid, substeps=1, weights=(3,)).weights == [3.0]
