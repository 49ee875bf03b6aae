"""Host-side tests of the vertical mixing diffusivities (no GPU): the export list of libtripolar_hip_mixing.so, which is staged beside the
table of the libraries as a target of its own; every argument error of the two entry points in the order their header gives (status and
message; every call below fails in validation, none reaches a launch, the pointers are fabricated and never dereferenced: a call that
passes a check is refused by a later one, at the latest by the stencil check, the sixth, at halo (0, 0, 0)); every refusal and record of the
Python layer on host-only grid records; the loader; what `make -n` prints for the new target; that build() names it; the build records."""
import inspect
import json
import math
import os
import re
import subprocess

import pytest

from test_abi import ROOT, exported_symbols
from test_weno_momentum_conditions import _grid

CSRC = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
STAGED = os.path.join(CSRC, "staged")
NAMES = ["tpg_convective_adjustment_diffusivities", "tpg_mixing_last_error", "tpg_ri_based_diffusivities"]
G0 = (48, 40, 6, 0, 0, 0)                                          # Nx, Ny, Nz at halo (0, 0, 0): the stencil check refuses what passes the rest
CELLS, FACES = 48 * 40 * 6 * 8, 48 * 40 * 7 * 8
BASE = 1 << 32
B, U, V, KPREV, NPREV, KC, NC, KU, KV = (BASE + 4 * q * FACES for q in range(9))
DZF, NCC, NFC, NCF = (5 + q << 20 for q in range(4))
STENCIL = ("the rule reads b, u, v and the *_prev arrays one cell west, east, south and north of the interior: Hx >= 1 and Hy >= 1 needed "
           "(halo (0,0,0))")
WHY = " (every item reads its neighbours' cells while they write: the caller ping-pongs)"
CA_PARAMS = ("background_kappa", "convective_kappa", "background_nu", "convective_nu")
RI_PARAMS = ("nu0", "kappa0", "kappa_ca", "Ri0", "Ri_delta", "Cav")


def _header():
    text = open(os.path.join(STAGED, "tripolar_hip_mixing.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ca(b=B, kc=KC, nc=NC, ku=KU, kv=KV, params=(0.1, 1.0, 0.2, 2.0), dz_f=DZF, n_cc=NCC, n_fc=NFC, n_cf=NCF, value=0.0, geom=G0, ft=1, **named):
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    params = [named.get(k, x) for k, x in zip(CA_PARAMS, params)]
    return M.mixing_lib().tpg_convective_adjustment_diffusivities(b, kc, nc, ku, kv, *params, dz_f, n_cc, n_fc, n_cf, value, *geom, ft, None)


def _ri(b=B, u=U, v=V, kprev=KPREV, nprev=NPREV, kc=KC, nc=NC, ku=KU, kv=KV, params=(0.7, 0.5, 1.7, 0.1, 0.4, 0.6), dz_f=DZF, n_cc=NCC, n_fc=NFC,
        n_cf=NCF, value=0.0, geom=G0, ft=1, **named):
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    params = [named.get(k, x) for k, x in zip(RI_PARAMS, params)]
    return M.mixing_lib().tpg_ri_based_diffusivities(b, u, v, kprev, nprev, kc, nc, ku, kv, *params, dz_f, n_cc, n_fc, n_cf, value, *geom, ft, None)


def test_the_export_list():
    """literally: three names"""
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    M.mixing_lib()
    assert sorted(exported_symbols(M.MIXING_LIB_PATH)) == ["tpg_convective_adjustment_diffusivities", "tpg_mixing_last_error",
                                                            "tpg_ri_based_diffusivities"]


def test_header_map_exports_and_signatures_are_the_three_names(osg):
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    M.mixing_lib()
    _, code = _header()
    declared = sorted(set(re.findall(r"\b(tpg_[a-z0-9_]+)\s*\(", code)))
    text = open(os.path.join(STAGED, "mixing.map")).read()
    assert "local: *;" in text
    assert declared == NAMES == sorted(re.findall(r"\btpg_[a-z0-9_]+", text)) == sorted(exported_symbols(M.MIXING_LIB_PATH)) == sorted(M.MIXING_SIGNATURES)
    double = osg._lib.C.c_double
    _, ca = M.MIXING_SIGNATURES["tpg_convective_adjustment_diffusivities"]
    _, ri = M.MIXING_SIGNATURES["tpg_ri_based_diffusivities"]
    assert len(ca) == 22 and [q for q, t in enumerate(ca) if t is double] == [5, 6, 7, 8, 13]
    assert len(ri) == 28 and [q for q, t in enumerate(ri) if t is double] == [9, 10, 11, 12, 13, 14, 19]
    # the prototypes of the header have as many parameters
    for name, n in (("tpg_convective_adjustment_diffusivities", 22), ("tpg_ri_based_diffusivities", 28)):
        proto = re.search(name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        assert len(proto.split(",")) == n, name
    for other in osg._lib.LIBRARIES:                               # no name of it is in a library of the table
        path = getattr(osg._lib, osg._lib.LIBRARIES[other].path_global)
        assert not set(NAMES) & set(exported_symbols(path)), other
    assert len(osg._lib.LIBRARIES) == 15 and "mixing" not in osg._lib.LIBRARIES and not hasattr(osg._lib, "MIXING_SIGNATURES")


def test_library_reads_no_environment_variable():
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    M.mixing_lib()
    und = subprocess.run(["nm", "-D", "--undefined-only", M.MIXING_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und and "hipMalloc" not in und


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include "tripolar_hip_mixing.h"\ntypedef void (*fn)(void);\nstatic fn table[] = {' + ", ".join(f"(fn){n}" for n in NAMES)
                   + "};\nint main(void) { return sizeof(table) == 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", STAGED, "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text, _ = _header()
    assert "[recalled: Oceananigans'" in text and "parity unpinned" in text
    assert [c for c in re.findall(r"#define (TPG_[A-Z0-9_]+)", text) if not c.endswith("_H")] == []


def test_missing_library_fails_loudly(osg, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the binding and the plan raise, and name the path they looked at"""
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    missing = str(tmp_path / os.path.basename(M.MIXING_LIB_PATH))
    monkeypatch.setattr(M, "_mixing", None)
    monkeypatch.setattr(M, "MIXING_LIB_PATH", missing)
    with pytest.raises(ImportError, match="only backend") as err:
        M.mixing_lib()
    assert missing in str(err.value)
    grid = _grid(osg)
    with pytest.raises(ImportError, match="only backend"):
        osg.vertical_mixing_plan(osg.ConvectiveAdjustmentVerticalDiffusivity(convective_kappa_z=1.0), osg.CenterField(grid), fill_halos=False)


def test_argument_errors_without_device_work(osg):
    """the seven refusals of the header, in its order: each is reached only when everything before it passes"""
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    lib = M.mixing_lib()
    err = lambda: lib.tpg_mixing_last_error().decode()             # noqa: E731
    for call in (_ca, _ri):
        assert call() == -5 and err() == STENCIL                   # the base calls pass the first five checks
        # 1. the geometry (before the pointers)
        assert call(ft=7, b=None) == -1 and err() == "unknown element type ft=7"
        assert call(geom=(49, 40, 3, 4, 4, 4), b=None) == -2
        assert call(geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
        assert call(geom=(48, 4, 3, 4, 5, 4)) == -5 and err().startswith("halo (4,5) larger than size")
        # 2. the null combinations (before the numbers)
        assert call(b=None, dz_f=None, params=(math.nan,) * 6) == -1 and err() == "null b"
        assert call(dz_f=None, kc=None, nc=None, ku=None, kv=None) == -1 and err() == "null dz_f"
        assert call(kc=None, nc=None, ku=None, kv=None, params=(math.nan,) * 6) == -1 and err() == "no output: kappa_c, nu_c, kappa_u and kappa_v are all null"
        for one in ("kc", "nc", "ku", "kv"):                       # any one output is a call
            assert call(**{k: None for k in ("kc", "nc", "ku", "kv") if k != one}) == -5 and err() == STENCIL
        # 4. alignment (after the numbers, before the overlaps)
        for ft, off in ((1, 4), (0, 2)):
            assert call(b=B + off, kc=B, ft=ft) == -1 and err() == "b, u, v, kappa_c_prev or nu_c_prev pointer not aligned to its element type"
            for out in ("kc", "nc", "ku", "kv"):
                assert call(ft=ft, dz_f=DZF + off, **{out: B + off}) == -1 and err() == "kappa_c, nu_c, kappa_u or kappa_v pointer not aligned to its element type"
            assert call(ft=ft, dz_f=DZF + off, n_cc=NCC + 2) == -1 and err() == "dz_f pointer not aligned to its element type"
        for plane in ("n_cc", "n_fc", "n_cf"):
            assert call(kc=B, **{plane: NCC + 2}) == -1 and err() == "count plane pointer not aligned to int32"
        # 5. the overlaps: any output against any other array; identical, one element inside from either side; right behind or in front is none
        for shift, status in ((0, -1), (8, -1), (-8, -1), (CELLS - 8, -1), (8 - FACES, -1), (CELLS, -5), (-FACES, -5)):
            assert call(kc=B + shift) == status and err() == ("kappa_c overlaps b" + WHY if status == -1 else STENCIL), shift
        for shift, status in ((0, -1), (FACES - 8, -1), (8 - FACES, -1), (FACES, -5), (-FACES, -5)):
            assert call(ku=NC + shift) == status and err() == ("nu_c overlaps kappa_u" + WHY if status == -1 else STENCIL), shift
            assert call(kv=KC + shift) == status and err() == ("kappa_c overlaps kappa_v" + WHY if status == -1 else STENCIL), shift
        assert call(dz_f=KV + 8) == -1 and err() == "kappa_v overlaps dz_f" + WHY
        assert call(dz_f=KV + FACES) == -5 and err() == STENCIL
        assert call(n_fc=KU + FACES - 4) == -1 and err() == "kappa_u overlaps n_fc" + WHY
        assert call(n_cf=KV - 48 * 40 * 4) == -5 and err() == STENCIL
        assert call(nc=None, n_cc=NC) == -5 and err() == STENCIL   # an absent output overlaps nothing
        # 6. the stencil, whatever the outputs are
        for halo in ((0, 1, 1), (1, 0, 1), (0, 0, 4)):
            assert call(geom=(48, 40, 6, *halo), ku=None, kv=None) == -5 and err() == STENCIL.replace("(0,0,0)", "(%d,%d,%d)" % halo)
        # 7. more work items than 32 bits index: the plane check every entry point shares refuses every such geometry first
        assert call(geom=(65536, 32768, 1, 1, 1, 1), ft=0) == -5 and "32-bit" in err()
    # 2. the Ri call's own null combinations
    assert _ri(u=None, dz_f=None) == -1 and err() == "null u or v"
    assert _ri(v=None, kc=None, nc=None, ku=None, kv=None) == -1 and err() == "null u or v"
    assert _ri(nprev=None, Ri_delta=0.0) == -1 and err() == "kappa_c_prev without nu_c_prev: the time average takes both or neither"
    assert _ri(kprev=None, Ri_delta=0.0) == -1 and err() == "nu_c_prev without kappa_c_prev: the time average takes both or neither"
    assert _ri(kprev=None, nprev=None) == -5 and err() == STENCIL
    # 3. the numbers (before alignment), in the order of the argument list
    for call, names in ((_ca, CA_PARAMS), (_ri, RI_PARAMS)):
        for q, name in enumerate(names):
            for value in (math.nan, math.inf, -math.inf):
                later = {k: math.nan for k in names[q + 1:]}
                assert call(b=B + 4, value=math.nan, **{name: value}, **later) == -1 and err() == f"{name} is not finite", name
            assert call(ft=0, **{name: 1e300}) == -1 and err() == f"{name} is not finite"      # as the element type holds it
            assert call(ft=1, **{name: 1e300}) == -5 and err() == STENCIL
        for value in (math.nan, math.inf):
            assert call(value=value, b=B + 4) == -1 and err() == "mask_value is not finite"
            assert call(value=value, n_cc=None, n_fc=None, n_cf=None) == -5 and err() == STENCIL           # not looked at without a count plane
    for delta in (0.0, -0.4, -0.0):
        assert _ri(Ri_delta=delta, Cav=-1.0, b=B + 4) == -1 and err().startswith("Ri_delta = ") and "is not positive" in err(), delta
    assert _ri(Ri_delta=1e-60, ft=0) == -1 and "is not positive" in err()                   # a Float32 zero
    assert _ri(Ri_delta=1e-60, ft=1) == -5 and err() == STENCIL
    assert _ri(Cav=-1.0, b=B + 4) == -1 and err() == "1 + Cav == 0: the time average divides by it"
    assert _ri(Cav=-1.0 + 1e-12, ft=0) == -1 and err() == "1 + Cav == 0: the time average divides by it"   # formed in the element type
    assert _ri(Cav=-1.0 + 1e-12, ft=1) == -5 and err() == STENCIL
    assert _ri(Cav=-1.0, kprev=None, nprev=None) == -5 and err() == STENCIL                 # without the *_prev arrays Cav is not used
    # 4. the inputs of the Ri call
    for name in ("u", "v", "kprev", "nprev"):
        assert _ri(kc=B, **{name: U + 4}) == -1 and err() == "b, u, v, kappa_c_prev or nu_c_prev pointer not aligned to its element type"
    # 5. ... and their overlaps with an output
    for name, word in (("u", "u"), ("v", "v"), ("kprev", "kappa_c_prev"), ("nprev", "nu_c_prev")):
        assert _ri(**{name: KV + 16}) == -1 and err() == f"kappa_v overlaps {word}" + WHY
    assert _ri(u=B, v=B, kprev=NPREV) == -5 and err() == STENCIL   # inputs may share memory


def test_the_records_and_the_closures_refused_by_name(osg):
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    ri = osg.RiBasedVerticalDiffusivity()
    assert (ri.nu0, ri.kappa0, ri.kappa_ca, ri.Cen, ri.Cav, ri.Ri0, ri.Ri_delta) == (0.7, 0.5, 1.7, 0.1, 0.6, 0.1, 0.4)      # Oceananigans' [recalled]
    assert ri.Ri_dependent_tapering == osg.HyperbolicTangentRiDependentTapering() and ri.horizontal_Ri_filter is None
    assert isinstance(ri.time_discretization, osg.VerticallyImplicitTimeDiscretization)
    ca = osg.ConvectiveAdjustmentVerticalDiffusivity()
    assert (ca.convective_kappa_z, ca.convective_nu_z, ca.background_kappa_z, ca.background_nu_z) == (0.0, 0.0, 0.0, 0.0)
    grid = _grid(osg)
    b, u, v = osg.CenterField(grid), osg.XFaceField(grid), osg.YFaceField(grid)
    plan_of = lambda c: osg.vertical_mixing_plan(c, b, u, v, fill_halos=False)      # noqa: E731
    linear = osg.PiecewiseLinearRiDependentTapering()
    with pytest.raises(NotImplementedError, match="HyperbolicTangentRiDependentTapering is not built") as e:
        plan_of(ri)                                                # the record's defaults are refused at plan time, with what is built
    assert M.BUILT in str(e.value) and "PiecewiseLinearRiDependentTapering()" in M.BUILT and "Cen=0" in M.BUILT
    with pytest.raises(NotImplementedError, match="ExponentialRiDependentTapering is not built") as e:
        plan_of(osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=osg.ExponentialRiDependentTapering(), Cen=0))
    assert M.BUILT in str(e.value)
    with pytest.raises(NotImplementedError, match=r"the entrainment term \(Cen = 0.1\) is not built") as e:
        plan_of(osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=linear))
    assert M.BUILT in str(e.value)
    with pytest.raises(NotImplementedError, match="the horizontal Ri filter 'FivePointHorizontalFilter' is not built") as e:
        plan_of(osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=linear, Cen=0, horizontal_Ri_filter="FivePointHorizontalFilter"))
    assert M.BUILT in str(e.value)
    with pytest.raises(NotImplementedError, match="ExplicitTimeDiscretization.* is not built"):
        plan_of(osg.RiBasedVerticalDiffusivity(osg.ExplicitTimeDiscretization(), Ri_dependent_tapering=linear, Cen=0))
    with pytest.raises(NotImplementedError, match="CATKEVerticalDiffusivity is not built"):
        plan_of(type("CATKEVerticalDiffusivity", (), {})())
    with pytest.raises(NotImplementedError, match="VerticalScalarDiffusivity is not built as a vertical mixing closure"):
        plan_of(osg.VerticalScalarDiffusivity())
    with pytest.raises(NotImplementedError, match="kappa0 = .* is not built: every parameter of the closure is one number"):
        plan_of(osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=linear, Cen=0, kappa0=osg.CenterField(grid)))
    with pytest.raises(ValueError, match="Ri_delta = 0.0 must be positive"):
        plan_of(osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=linear, Cen=0, Ri_delta=0.0))
    with pytest.raises(ValueError, match="nu0 = nan is not finite"):
        plan_of(osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=linear, Cen=0, nu0=math.nan))
    # the older modules still refuse these closures by name: their messages are pinned and out of date
    with pytest.raises(NotImplementedError, match="ConvectiveAdjustmentVerticalDiffusivity is not built"):
        osg.implicit_step_plan(u, v, [b], ca, 1.0)


def test_python_refusals_and_plans_on_host_grids(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    from orthogonalsphericalshellgrids.jl_amd._operator_plan import OperatorPlan
    for name in ("ConvectiveAdjustmentVerticalDiffusivity", "RiBasedVerticalDiffusivity", "PiecewiseLinearRiDependentTapering",
                 "HyperbolicTangentRiDependentTapering", "ExponentialRiDependentTapering", "vertical_mixing_diffusivities", "vertical_mixing_plan",
                 "VerticalMixingPlan", "mixed_implicit_step_plan", "MixedImplicitStepPlan"):
        assert hasattr(osg, name), name
    assert issubclass(osg.VerticalMixingPlan, OperatorPlan)
    grid, other = _grid(osg), _grid(osg)
    b, u, v, w = osg.CenterField(grid), osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    ca = osg.ConvectiveAdjustmentVerticalDiffusivity(convective_kappa_z=1.5, convective_nu_z=2.5, background_kappa_z=0.01, background_nu_z=0.02)
    steady = osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=osg.PiecewiseLinearRiDependentTapering(), Cen=0, Cav=0)
    averaged = osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=osg.PiecewiseLinearRiDependentTapering(), Cen=0)
    plan_of = osg.vertical_mixing_plan
    with pytest.raises(TypeError, match=r"b must be a Field at \(Center, Center, Center\)"):
        plan_of(ca, u, fill_halos=False)
    with pytest.raises(TypeError, match="reads b alone: u and v must be None"):
        plan_of(ca, b, u, v, fill_halos=False)
    with pytest.raises(TypeError, match="RiBasedVerticalDiffusivity needs u and v"):
        plan_of(steady, b, fill_halos=False)
    with pytest.raises(TypeError, match=r"v must be a Field at \(Center, Face, Center\)"):
        plan_of(steady, b, u, u, fill_halos=False)
    with pytest.raises(TypeError, match=r"kappa_u must be a Field at \(Face, Center, Face\)"):
        plan_of(ca, b, kappa_u=w, fill_halos=False)
    with pytest.raises(ValueError, match="one grid"):
        plan_of(ca, b, kappa_c=osg.ZFaceField(other), fill_halos=False)
    with pytest.raises(TypeError, match="no output"):
        plan_of(ca, b, kappa_c=None, nu_c=None, kappa_u=None, kappa_v=None, fill_halos=False)
    with pytest.raises(ValueError, match="two outputs are one field"):
        plan_of(ca, b, kappa_c=w, nu_c=osg.ZFaceField(grid, data=w.data), fill_halos=False)
    with pytest.raises(ValueError, match=r"Hx and Hy must be at least 1 \(halo \(0, 3, 1\)\)"):
        plan_of(ca, osg.CenterField(_grid(osg, halo=(0, 3, 1))), fill_halos=False)
    with pytest.raises(TypeError, match=r"the time average \(Cav = 0.6\) reads the previous kappa_c and nu_c"):
        plan_of(averaged, b, u, v, nu_c=None)
    with pytest.raises(TypeError, match=r"the time average \(Cav = 0.6\)"):
        plan_of(averaged, b, u, v, fill_halos=False)
    band = _grid(osg)
    band.global_size = (8, 12, 3)
    with pytest.raises(NotImplementedError, match="latitude-band grids are not handled"):
        plan_of(ca, osg.CenterField(band), fill_halos=False)
    # the plans on a host-only record: built, never called
    p = plan_of(ca, b, kappa_v=None, fill_halos=False)
    fn, a = p._call
    assert fn is M.mixing_lib().tpg_convective_adjustment_diffusivities and len(a) == 21
    assert a[0] == b.data.data_ptr() and a[1] == p.outputs["kappa_c"].data.data_ptr() and a[3] == p.outputs["kappa_u"].data.data_ptr() and a[4] is None
    assert a[5:9] == (0.01, 1.5, 0.02, 2.5) and a[9] is not None and a[10:13] == (None,) * 3 and a[14:] == (8, 6, 3, 3, 3, 1, 1)
    assert p.outputs["kappa_v"] is None and p.outputs["kappa_u"].loc == (osg.Face, osg.Center, osg.Face) and p.twins is None
    assert tuple(p.outputs["kappa_c"].data.shape) == (3 + 1 + 2, 6 + 6, 8 + 6)
    r = plan_of(steady, b, u, v, kappa_c=w, fill_halos=False)
    fn, a = r._call
    assert fn is M.mixing_lib().tpg_ri_based_diffusivities and len(a) == 27 and a[3:5] == (None, None) and a[5] == w.data.data_ptr()
    assert a[9:15] == (0.7, 0.5, 1.7, 0.1, 0.4, 0.0) and r.outputs["kappa_c"] is w and not r.averaged
    one_shot = inspect.signature(osg.vertical_mixing_diffusivities)
    assert list(one_shot.parameters)[:4] == ["closure", "b", "u", "v"]
    # the step: the diffusivity call, then u, v and the tracers in the FIELD form, sharing one scratch
    T, S = osg.CenterField(grid), osg.CenterField(grid)
    step = osg.mixed_implicit_step_plan(ca, u, v, {"T": T, "S": S}, T, 0.5, path="on_chip")
    assert [type(x).__name__ for x in step.plans] == ["VerticalImplicitDiffusionPlan"] * 3 and step.dt == 0.5
    assert step.mixing.outputs["nu_c"] is None                     # convective adjustment: nothing reads it
    for plan, key, n in zip(step.plans, ("kappa_u", "kappa_v", "kappa_c"), (1, 1, 2)):
        args = plan._call[1]
        assert args[1] == n and args[2] == step.mixing.outputs[key].data.data_ptr() and args[4] == osg._lib.TPG_KAPPA_FIELD and args[9] == 0.5
    again = step.with_dt(0.25)
    assert again.mixing is step.mixing and [x._call[1][9] for x in again.plans] == [0.25] * 3 and again.dt == 0.25
    assert [x._call[1][:9] for x in again.plans] == [x._call[1][:9] for x in step.plans]
    with pytest.raises(TypeError, match="RiBasedVerticalDiffusivity needs u and v"):
        osg.mixed_implicit_step_plan(steady, None, None, [T], T, 0.5)
    with pytest.raises(TypeError, match="no fields"):
        osg.mixed_implicit_step_plan(ca, None, None, [], T, 0.5)
    with pytest.raises(NotImplementedError, match="HyperbolicTangentRiDependentTapering is not built"):
        osg.mixed_implicit_step_plan(osg.RiBasedVerticalDiffusivity(), u, v, [T], T, 0.5)
    tracers_only = osg.mixed_implicit_step_plan(ca, None, None, [T], T, 0.5, path="on_chip")
    assert len(tracers_only.plans) == 1 and tracers_only.mixing.outputs["kappa_u"] is None
    assert torch.is_tensor(tracers_only.mixing.outputs["kappa_c"].data)


def test_the_new_target_of_the_staged_makefile():
    """`make mixing` prints one compile line, one link line and the rename, with the flags of the first library; the default target does not
    reach it (what that prints is pinned by tests/test_diffusion_conditions.py)"""
    lines = [line for line in subprocess.run(["make", "-n", "-B", "-C", STAGED, "mixing", "MIXING_TAG=_t", "MIXING_FLAGS=-DTPG_X=1", "HIPCC=hipcc", "ARCH=gfx950"],
                                             capture_output=True, text=True, check=True).stdout.splitlines() if not line.startswith("make")]
    compiles = [line for line in lines if " -c " in line and "tpg_api" not in line]
    assert len(compiles) == 1 and compiles[0].endswith("-c tpg_mixing.hip -o tpg_mixing_t.o") and "diffusion" not in compiles[0]
    assert " -DTPG_X=1 " in compiles[0] and " -ffp-contract=off " in compiles[0] and " --offload-arch=gfx950 " in compiles[0] and " -I .. " in compiles[0]
    links = [line for line in lines if "-shared" in line]
    assert len(links) == 1 and " -Wl,--version-script=mixing.map " in links[0]
    assert links[0].endswith("-o ../../libtripolar_hip_mixing_t.so.tmp ../tpg_api.o tpg_mixing_t.o")
    assert lines[-1] == "mv -f ../../libtripolar_hip_mixing_t.so.tmp ../../libtripolar_hip_mixing_t.so"
    default = subprocess.run(["make", "-n", "-B", "-C", STAGED], capture_output=True, text=True, check=True).stdout
    assert "mixing" not in default
    table = subprocess.run(["make", "-n", "-B", "-C", CSRC], capture_output=True, text=True, check=True).stdout
    assert "mixing" not in table and "staged" not in table
    body = open(os.path.join(STAGED, "tpg_mixing.hip")).read()
    assert '#include "tpg_operator.hpp"' in body and "chunk_plan<T>" in body and "getenv" not in body and "store_chunk<NT>" in body
    assert body.count("__global__") == 1 and "__syncthreads" not in body and "atomic" not in body.lower() and "hipMalloc" not in body
    assert "__shared__" not in body


def test_build_names_the_new_target():
    import __graft_entry__
    source = inspect.getsource(__graft_entry__.build)
    assert '["make", "-C", os.path.join(csrc, "staged"), "mixing"]' in source and "mixing.mixing_lib()" in source
    assert "*.so" in open(os.path.join(ROOT, ".gitignore")).read().split()     # the library is a build product


def test_the_sanitizer_program_of_the_host_checks_builds_and_passes(tmp_path):
    """tools/mixing_argcheck.cpp, a stand-alone host program with its own main, built as its header comment says with the address and
    undefined-behaviour sanitizers on the host side and run here, on the CPU: it exits 0 and prints its one line"""
    tool = open(os.path.join(ROOT, "tools", "mixing_argcheck.cpp")).read()
    assert "int main()" in tool and "-fsanitize=address,undefined" in tool and "tpg_ri_based_diffusivities(" in tool
    exe = str(tmp_path / "mixing_argcheck")
    build = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                            "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tools", "mixing_argcheck.cpp"), os.path.join(STAGED, "tpg_mixing.hip"), os.path.join(CSRC, "tpg_api.hip"),
                            "-ldl", "-o", exe], capture_output=True, text=True, cwd=str(tmp_path))
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "mixing_argcheck: every call refused in validation, with its status and message", run.stdout + run.stderr


def test_the_records_of_the_build():
    """nothing differs in an existing object; nothing of the new kernels in private memory, no LDS, no register spill"""
    diff = json.load(open(os.path.join(ROOT, "profiles", "mixing", "isa_diff.json")))
    assert "tpg_vertical_diffusion.o" in diff and "tpg_grid.o" in diff and "staged/tpg_diffusion.o" in diff and len(diff) >= 28
    for name, r in diff.items():
        assert r.get("code_object_identical", True), name
        assert not any(r.get(k) for k in ("differing", "metadata_differing", "only_old", "only_new", "renamed")), name
    res = json.load(open(os.path.join(ROOT, "profiles", "mixing", "resources.json")))["kernels"]
    assert len(res) == 10 and all("k_mixing_diffusivities" in k for k in res)        # 5 chunk forms x 2 closures
    for k, r in res.items():
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"], r["group_segment_fixed_size"],
                r["uses_dynamic_stack"]) == ("0", "0", "0", "0", "false"), k
        assert int(r["vgpr_count"]) + int(r["agpr_count"]) <= 256 and int(r["max_flat_workgroup_size"]) == 256, k
