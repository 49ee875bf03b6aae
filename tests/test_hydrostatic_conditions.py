"""Host-side tests of the Coriolis and hydrostatic pressure-gradient tendencies (no GPU): the export list of libtripolar_hip_hydrostatic.so,
every argument error of tpg_hydrostatic_tendencies in the order the header gives (status and message; every call below fails in
validation, none reaches a launch, the pointers are fabricated and never dereferenced), every refusal of the Python layer on host-only grid
records, the records, coriolis_parameter, the loader, and the names the build is made of."""
import dataclasses
import json
import math
import os

import pytest

from test_weno_momentum_conditions import BASE, FAR, G, NCF, NFC, PARENT, PLANE, _grid as _record

NAMES = ["tpg_hydrostatic_last_error", "tpg_hydrostatic_tendencies"]
U, V, B = BASE, BASE + PARENT, BASE + 2 * PARENT
GU, GV, P = FAR, FAR + 3 * PARENT, FAR + 6 * PARENT
PLANES = ("f_ff", "dx_fc", "dy_fc", "dx_cf", "dy_cf", "dz_f")
AT = {name: (q + 1) << 20 for q, name in enumerate(PLANES)}
HALO = "the rule reads u, v, b[i-1..i+1, j-1..j+1] and b[k..Nz+1]: Hx >= 1, Hy >= 1 and Hz >= 1 needed (halo ({},{},{}))"
COUNTS = "the count planes n_fc and n_cf are given together or not at all ({} is null)"
WHY = " (every item reads cells while its neighbours write)"


def _call(lib, n_fc=None, n_cf=None, geom=G, ft=1, scheme=0, mode=0, **over):
    s = dict(u=U, v=V, b=B, Gu=GU, Gv=GV, p_out=P, **AT)
    s.update(over)
    return lib.tpg_hydrostatic_tendencies(*s.values(), n_fc, n_cf, 0.0, scheme, mode, *geom, ft, None)


def _grid(osg, halo=(1, 1, 1), **kw):
    """test_weno_momentum_conditions' host-only grid record, with a phi_ff plane running from -80 to 80 degrees, symmetric about 0"""
    import torch
    Hx, Hy, Hz = halo
    rows = torch.linspace(-80, 80, 6 + 2 * Hy, dtype=torch.float64)
    arrays = {"lambda_cc": torch.zeros(6 + 2 * Hy, 8 + 2 * Hx, dtype=torch.float64), "phi_ff": rows[:, None].expand(-1, 8 + 2 * Hx).contiguous()}
    return _record(osg, halo, arrays=arrays, **kw)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import ROOT, declared_symbols, exported_symbols
    L = osg._lib
    L.hydrostatic_lib()
    assert sorted(declared_symbols("tripolar_hip_hydrostatic.h")) == NAMES == sorted(exported_symbols(L.HYDROSTATIC_LIB_PATH)) == sorted(L.HYDROSTATIC_SIGNATURES)
    restype, argtypes = L.HYDROSTATIC_SIGNATURES["tpg_hydrostatic_tendencies"]
    assert len(argtypes) == 25 and argtypes[14] is L.C.c_double and argtypes[:14] == [L.C.c_void_p] * 14


def test_argument_errors_without_device_work(osg):
    """the nine refusals of the header, in its order: each is reached only when everything before it passes"""
    lib = osg._lib.hydrostatic_lib()
    err = lambda: lib.tpg_hydrostatic_last_error().decode()       # noqa: E731
    # 1. the geometry (before a bad scheme)
    assert _call(lib, ft=7, scheme=9) == -1 and err() == "unknown element type ft=7"
    assert _call(lib, geom=(49, 40, 3, 4, 4, 4)) == -2
    assert _call(lib, geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert _call(lib, geom=(48, 40, 3, 4, 4, -1)) == -1 and err().startswith("invalid size")
    # 2. the scheme, then the mode (before the pointers)
    for scheme in (2, -1, 7):
        assert _call(lib, scheme=scheme, mode=9, f_ff=None, b=None) == -5
        assert err().startswith(f"Coriolis scheme {scheme} is not built") and "ActiveCellEnstrophyConserving is not" in err()
    for mode in (2, -1):
        assert _call(lib, mode=mode, f_ff=None, b=None) == -5 and err().startswith(f"tendency mode {mode} is not built")
    for scheme, mode in ((0, 0), (0, 1), (1, 0), (1, 1)):          # the four that are: the call goes on to the halo check
        assert _call(lib, scheme=scheme, mode=mode, geom=(48, 40, 3, 4, 4, 0)) == -5 and err() == HALO.format(4, 4, 0)
    # 3. neither term
    assert _call(lib, f_ff=None, b=None, Gu=None) == -1 and err() == "neither f_ff nor b: no term to compute"
    # 4. the null combinations, in this order
    assert _call(lib, Gu=None, p_out=None) == -1 and err() == "Gu and Gv are given together or not at all (Gu is null)"
    assert _call(lib, Gv=None, dx_fc=None) == -1 and err() == "Gu and Gv are given together or not at all (Gv is null)"
    for over in (dict(b=None), dict(p_out=None)):
        assert _call(lib, Gu=None, Gv=None, **over) == -1 and err() == "without Gu and Gv the call is the pressure alone: b and p_out needed"
    assert _call(lib, b=None, dx_fc=None) == -1 and err() == "p_out without b"
    for name in ("dx_fc", "dy_cf"):
        assert _call(lib, u=None, **{name: None}) == -1 and err() == "null dx_fc or dy_cf"
    for name in ("u", "v", "dx_cf", "dy_fc"):
        assert _call(lib, dz_f=None, **{name: None}) == -1 and err() == "f_ff without u, v, dx_cf or dy_fc"
    assert _call(lib, dz_f=None, n_fc=NFC) == -1 and err() == "b without dz_f"
    # what a dropped term does not need may be null: the calls go on to the halo check
    h0 = (48, 40, 3, 4, 4, 0)
    assert _call(lib, geom=h0, f_ff=None, u=None, v=None, dx_cf=None, dy_fc=None) == -5 and err() == HALO.format(4, 4, 0)
    assert _call(lib, geom=h0, b=None, p_out=None, dz_f=None) == -5 and err() == HALO.format(4, 4, 0)
    assert _call(lib, geom=h0, Gu=None, Gv=None, f_ff=None, u=None, v=None, dx_fc=None, dy_fc=None, dx_cf=None, dy_cf=None) == -5 and err() == HALO.format(4, 4, 0)
    # 5. one count plane without the other
    assert _call(lib, n_fc=NFC, u=U + 4) == -1 and err() == COUNTS.format("n_cf")
    assert _call(lib, n_cf=NCF) == -1 and err() == COUNTS.format("n_fc")
    # 6. alignment: to the element type, Float64 and Float32, and the count planes to int32
    for name, at in (("u", U), ("v", V), ("b", B)):
        assert _call(lib, Gu=GU + 4, **{name: at + 4}) == -1 and err() == "u, v or b pointer not aligned to its element type"
        assert _call(lib, ft=0, **{name: at + 2}) == -1 and err() == "u, v or b pointer not aligned to its element type"
    for name, at in (("Gu", GU), ("Gv", GV), ("p_out", P)):
        assert _call(lib, f_ff=AT["f_ff"] + 4, **{name: at + 4}) == -1 and err() == "Gu, Gv or p_out pointer not aligned to its element type"
        assert _call(lib, ft=0, **{name: at + 2}) == -1 and err() == "Gu, Gv or p_out pointer not aligned to its element type"
    for name in PLANES:
        assert _call(lib, n_fc=NFC + 2, n_cf=NCF, **{name: AT[name] + 4}) == -1 and err() == "f_ff, dx_fc, dy_fc, dx_cf, dy_cf or dz_f pointer not aligned to its element type"
        assert _call(lib, ft=0, **{name: AT[name] + 2}) == -1 and err().startswith("f_ff, dx_fc")
    assert _call(lib, n_fc=NFC + 2, n_cf=NCF, Gv=GU) == -1 and err() == "count plane pointer not aligned to int32"
    assert _call(lib, n_fc=NFC, n_cf=NCF + 2) == -1 and err() == "count plane pointer not aligned to int32"
    # 7. the overlaps: Gu, Gv and p_out against u, v, b and each other -- identical, one element inside from either side
    away = dict(u=3 * FAR, v=4 * FAR, b=5 * FAR)
    for shift in (0, 8, -8, PARENT - 8, 8 - PARENT):
        for out in ("Gu", "Gv", "p_out"):
            for name in ("u", "v", "b"):
                assert _call(lib, geom=h0 if shift == 0 else G, **{**away, name: BASE, out: BASE + shift}) == -1
                assert err() == f"{out} overlaps {name}" + WHY, (out, name, shift)
        assert _call(lib, Gv=GU + shift) == -1 and err() == "Gu overlaps Gv" + WHY
        assert _call(lib, p_out=GV + shift) == -1 and err() == "Gv overlaps p_out" + WHY
        assert _call(lib, p_out=GU + shift) == -1 and err() == "Gu overlaps p_out" + WHY
    p0 = PLANE * 3                                                 # exact: right behind or right in front is no overlap, one element nearer is
    for out in ("Gu", "Gv", "p_out"):
        for shift, status in ((p0, -5), (p0 - 8, -1), (-p0, -5), (8 - p0, -1)):
            assert _call(lib, geom=h0, **{**away, "b": BASE, out: BASE + shift}) == status, (out, shift)
            assert err() == (f"{out} overlaps b" + WHY if status == -1 else HALO.format(4, 4, 0))
    assert _call(lib, geom=h0, u=BASE, v=BASE, b=BASE) == -5         # u, v and b are only read: they may be one array
    # 8. the halo, one direction at a time, both types
    for geom in ((48, 40, 3, 0, 4, 4), (48, 40, 3, 4, 0, 4), (48, 40, 3, 4, 4, 0), (48, 40, 3, 0, 0, 0)):
        for ft in (0, 1):
            assert _call(lib, geom=geom, ft=ft, n_fc=NFC, n_cf=NCF) == -5 and err() == HALO.format(*geom[3:])
    assert _call(lib, geom=(2, 1, 1, 1, 1, 1), Gu=None) == -1        # the smallest shape passes the geometry (and is refused for what follows it)
    # 9. more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    assert _call(lib, geom=(65536, 32768, 1, 1, 1, 1), ft=0, u=1 << 44, v=2 << 44, b=3 << 44, Gu=4 << 44, Gv=5 << 44, p_out=6 << 44) == -5
    assert "32-bit" in err()


def test_the_records(osg):
    from orthogonalsphericalshellgrids.jl_amd import hydrostatic as hy
    c = osg.HydrostaticSphericalCoriolis()
    assert c.rotation_rate == 7.292115e-5 and c.scheme == osg.EnstrophyConserving() and hash(c) == hash(osg.HydrostaticSphericalCoriolis())
    assert osg.HydrostaticSphericalCoriolis(scheme=osg.EnergyConserving()) != c and osg.BuoyancyTracer() == osg.BuoyancyTracer()
    assert hy._refuse_coriolis(c, "x") == 0 and hy._refuse_coriolis(dataclasses.replace(c, scheme=osg.EnergyConserving()), "x") == 1
    ActiveCellEnstrophyConserving = type("ActiveCellEnstrophyConserving", (), {})
    with pytest.raises(NotImplementedError, match="the Coriolis scheme ActiveCellEnstrophyConserving is not built") as e:
        hy._refuse_coriolis(dataclasses.replace(c, scheme=ActiveCellEnstrophyConserving()), "x")
    assert "EnstrophyConserving()" in str(e.value) and "EnergyConserving()" in str(e.value) and "BuoyancyTracer()" in str(e.value)
    for name in ("FPlane", "BetaPlane"):
        with pytest.raises(NotImplementedError, match=f"{name} is not built: pass a padded \\(Face, Face\\) plane of f"):
            hy._refuse_coriolis(type(name, (), {})(), "x")
    with pytest.raises(NotImplementedError, match="coriolis 'hydrostatic' is not built"):
        hy._refuse_coriolis("hydrostatic", "x")
    assert hy.refuse_buoyancy(None) is None and hy.refuse_buoyancy(osg.BuoyancyTracer()) == osg.BuoyancyTracer()
    for name in ("SeawaterBuoyancy", "LinearEquationOfState", "TEOS10EquationOfState"):
        with pytest.raises(NotImplementedError, match=f"{name} is not built: SeawaterBuoyancy and the equations of state are out of scope") as e:
            hy.refuse_buoyancy(type(name, (), {})())
        assert "computes b from T and S itself" in str(e.value)


def test_coriolis_parameter(osg):
    """odd in phi, bounded by 2 Omega, cached per (grid, type, device), and at a handful of nodes what math.sin gives on the same Float64
    argument phi * (pi / 180).  The bound: both sines are within 1 ulp of the true value (what the two libraries claim), so they differ by at
    most 2 ulp <= 2 eps |sin|; the product with 2 Omega (the doubling is exact) rounds once on either side: eps / 2 each.  3 eps |f| in all;
    the test allows 4 eps |f|.  Rounded to Float32 it is the Float64 plane rounded once"""
    import torch
    grid = _grid(osg, (2, 2, 1))
    record = osg.HydrostaticSphericalCoriolis()
    f = osg.coriolis_parameter(grid, record)
    phi = grid.arrays["phi_ff"]
    assert f.shape == phi.shape and f.dtype == torch.float64 and f.device == phi.device
    assert torch.equal(f, -f.flip(0)) and float(f.abs().max()) <= 2 * record.rotation_rate and float(f[0, 0]) < 0 < float(f[-1, 0])
    eps = 2.0 ** -52
    for j in range(phi.shape[0]):
        want = 2 * record.rotation_rate * math.sin(float(phi[j, 3]) * (math.pi / 180))
        assert abs(float(f[j, 3]) - want) <= 4 * eps * abs(want), (j, float(f[j, 3]), want)
    assert osg.coriolis_parameter(grid, record) is f and osg.coriolis_parameter(grid) is f                   # cached with the grid
    f32 = osg.coriolis_parameter(grid, record, torch.float32)
    assert f32.dtype == torch.float32 and torch.equal(f32, f.to(torch.float32)) and osg.coriolis_parameter(grid, record, torch.float32) is f32
    slow = osg.coriolis_parameter(grid, dataclasses.replace(record, rotation_rate=1e-5))
    assert slow is not f and torch.allclose(slow * 7.292115, f)
    assert osg.coriolis_parameter(_grid(osg, (2, 2, 1)), record) is not f                                     # another grid, another plane
    with pytest.raises(NotImplementedError, match="FPlane is not built"):
        osg.coriolis_parameter(grid, type("FPlane", (), {})())


def test_python_refusals(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd._operator_plan import OperatorPlan
    for name in ("hydrostatic_tendencies", "hydrostatic_tendencies_plan", "HydrostaticTendenciesPlan", "update_hydrostatic_pressure",
                 "coriolis_parameter", "HydrostaticSphericalCoriolis", "BuoyancyTracer", "HydrostaticPressurePlan"):
        assert hasattr(osg, name), name
    for name in ("hydrostatic_lib", "check_hydrostatic", "HYDROSTATIC_SIGNATURES", "HYDROSTATIC_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    assert issubclass(osg.HydrostaticTendenciesPlan, OperatorPlan) and issubclass(osg.HydrostaticPressurePlan, OperatorPlan)
    grid, other = _grid(osg), _grid(osg)
    u, v, Gu, Gv = osg.XFaceField(grid), osg.YFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid)
    b, p = osg.CenterField(grid), osg.CenterField(grid)
    cor = osg.HydrostaticSphericalCoriolis()
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))       # noqa: E731
    window = (slice(None), slice(None), range(1, 3))
    for fn in (osg.hydrostatic_tendencies_plan, osg.hydrostatic_tendencies):
        with pytest.raises(ValueError, match="neither coriolis nor b"):
            fn(u, v, Gu, Gv)
        with pytest.raises(ValueError, match="pressure without b"):
            fn(u, v, Gu, Gv, coriolis=cor, pressure=p)
        with pytest.raises(NotImplementedError, match="BetaPlane is not built"):
            fn(u, v, Gu, Gv, coriolis=type("BetaPlane", (), {})())
        with pytest.raises(NotImplementedError, match="ActiveCellEnstrophyConserving is not built"):
            fn(u, v, Gu, Gv, coriolis=dataclasses.replace(cor, scheme=type("ActiveCellEnstrophyConserving", (), {})()))
        # locations
        with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
            fn(v, v, Gu, Gv, coriolis=cor)
        with pytest.raises(TypeError, match=r"v must be a Field at \(Center, Face, Center\)"):
            fn(u, b, Gu, Gv, coriolis=cor)
        with pytest.raises(TypeError, match=r"Gu must be a Field at \(Face, Center, Center\)"):
            fn(u, v, Gv, Gv, coriolis=cor)
        with pytest.raises(TypeError, match=r"Gv must be a Field at \(Center, Face, Center\)"):
            fn(u, v, Gu, Gu.data, coriolis=cor)
        with pytest.raises(TypeError, match=r"b must be a Field at \(Center, Center, Center\)"):
            fn(u, v, Gu, Gv, b=u)
        with pytest.raises(TypeError, match=r"pressure must be a Field at \(Center, Center, Center\)"):
            fn(u, v, Gu, Gv, b=b, pressure=v)
        # one grid, one type, no z-window: for every field of the call
        base = dict(u=u, v=v, Gu=Gu, Gv=Gv)
        makers = dict(u=osg.XFaceField, v=osg.YFaceField, Gu=osg.XFaceField, Gv=osg.YFaceField, b=osg.CenterField, pressure=osg.CenterField)
        for name in ("v", "Gu", "Gv", "b", "pressure"):
            pos, kw = dict(base), dict(b=b, pressure=p)
            (pos if name in pos else kw)[name] = makers[name](other)
            with pytest.raises(ValueError, match="one grid"):
                fn(*pos.values(), **kw)
            pos, kw = dict(base), dict(b=b, pressure=p)
            (pos if name in pos else kw)[name] = f32(makers[name])
            with pytest.raises(ValueError, match="one element type"):
                fn(*pos.values(), **kw)
        for name in makers:
            pos, kw = dict(base), dict(b=b, pressure=p)
            (pos if name in pos else kw)[name] = makers[name](grid, indices=window)
            with pytest.raises(NotImplementedError, match="z-windowed"):
                fn(*pos.values(), **kw)
        # aliases, by identity
        with pytest.raises(ValueError, match="Gu is u itself"):
            fn(u, v, u, Gv, coriolis=cor)
        with pytest.raises(ValueError, match="Gv is v itself"):
            fn(u, v, Gu, osg.YFaceField(grid, data=v.data), coriolis=cor)
        with pytest.raises(ValueError, match="pressure is b itself"):
            fn(u, v, Gu, Gv, b=b, pressure=b)
        with pytest.raises(ValueError, match="Gu and Gv are one field"):
            fn(u, v, Gu, osg.YFaceField(grid, data=Gu.data), coriolis=cor)
        # a plane of f of another shape or type
        with pytest.raises(ValueError, match=r"the plane of f must be a padded \(Face, Face\) plane of shape \(8, 10\)"):
            fn(u, v, Gu, Gv, coriolis=torch.zeros(6, 8, dtype=torch.float64))
        with pytest.raises(ValueError, match="the plane of f must be"):
            fn(u, v, Gu, Gv, coriolis=(torch.zeros(8, 10, dtype=torch.float32), osg.EnergyConserving()))
        # a halo below 1, one direction at a time: the message names the halo passed
        for halo in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
            thin = _grid(osg, halo)
            with pytest.raises(ValueError, match=r"every halo must be at least 1 \(halo \(%d, %d, %d\)\)" % halo):
                fn(osg.XFaceField(thin), osg.YFaceField(thin), osg.XFaceField(thin), osg.YFaceField(thin), b=osg.CenterField(thin))
        # a latitude band
        band = _grid(osg, topology=(osg.PeriodicTopology, osg.FullyConnected, osg.Bounded), global_size=(8, 12, 3), jrange=(1, 6))
        with pytest.raises(NotImplementedError, match="rows 0 and Ny \\+ 1 of a band are exchanged halo rows, and the band path .* is not tested yet"):
            fn(osg.XFaceField(band), osg.YFaceField(band), osg.XFaceField(band), osg.YFaceField(band), coriolis=cor)
    # the pressure alone
    with pytest.raises(TypeError, match=r"b must be a Field at \(Center, Center, Center\)"):
        osg.update_hydrostatic_pressure(u)
    with pytest.raises(TypeError, match=r"out must be a Field at \(Center, Center, Center\)"):
        osg.update_hydrostatic_pressure(b, out=u)
    with pytest.raises(ValueError, match="out is b itself"):
        osg.update_hydrostatic_pressure(b, out=b)
    with pytest.raises(ValueError, match="one grid"):
        osg.update_hydrostatic_pressure(b, out=osg.CenterField(other))
    thin = _grid(osg, (1, 1, 0))
    with pytest.raises(ValueError, match=r"every halo must be at least 1 \(halo \(1, 1, 0\)\)"):
        osg.update_hydrostatic_pressure(osg.CenterField(thin))


def test_missing_library_fails_loudly(osg, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the plan raises: it computes nothing some other way"""
    missing = str(tmp_path / os.path.basename(osg._lib.HYDROSTATIC_LIB_PATH))
    monkeypatch.setattr(osg._lib, "_hydrostatic", None)
    monkeypatch.setattr(osg._lib, "HYDROSTATIC_LIB_PATH", missing)
    grid = _grid(osg)
    with pytest.raises(ImportError, match="only backend"):
        osg.hydrostatic_tendencies_plan(osg.XFaceField(grid), osg.YFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid), b=osg.CenterField(grid))


def test_the_build_names_the_library_the_map_and_its_records():
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
    text = open(os.path.join(csrc, "hydrostatic.map")).read()
    assert all(n in text for n in NAMES) and "local: *;" in text
    body = open(os.path.join(csrc, "tpg_hydrostatic.hip")).read()
    assert '#include "tpg_operator.hpp"' in body and "check_overlaps(" in body and "chunk_plan<T>" in body and "getenv" not in body
    assert body.count("__global__") == 1 and "__shared__" not in body and "atomic" not in body.replace("No atomics", "")
    # the record of the build: nothing differs in an existing object; no scratch, no LDS, no spill in a committed instantiation
    diff = json.load(open(os.path.join(ROOT, "profiles", "hydrostatic", "isa_diff.json")))
    assert "tpg_momentum.o" in diff and "tpg_weno_vs.o" in diff and "tpg_grid.o" in diff and len(diff) >= 25
    for name, r in diff.items():
        assert not any(r.get(k) for k in ("differing", "metadata_differing", "only_old", "only_new", "renamed")), name
    res = json.load(open(os.path.join(ROOT, "profiles", "hydrostatic", "resources.json")))["kernels"]
    assert len(res) == 25 and all("k_hydrostatic_tendencies" in k for k in res)     # 5 chunk forms x (3 Coriolis forms x 2 - the empty one)
    for k, r in res.items():
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"], r["group_segment_fixed_size"]) == ("0", "0", "0", "0"), k
        assert int(r["vgpr_count"]) <= 512, k
