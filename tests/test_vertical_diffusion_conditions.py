"""Host-side tests of the vertically implicit diffusion step (no GPU): the export list of libtripolar_hip_vertical_diffusion.so, every
argument error of tpg_vertical_implicit_diffusion in the order the header gives (status and message; every call below fails in validation,
none reaches a launch, the pointers are fabricated and never dereferenced: a call that passes a check has 200 levels on the on-chip path and
is refused for the on-chip bound, the eighth check), tpg_vertical_diffusion_on_chip_levels, every refusal and record of the Python layer on
host-only grid records, the loader, and the names the build is made of."""
import json
import math
import os

import pytest

from test_weno_momentum_conditions import _grid

NAMES = ["tpg_vertical_diffusion_last_error", "tpg_vertical_diffusion_on_chip_levels", "tpg_vertical_implicit_diffusion"]
G = (48, 40, 200, 4, 4, 4)                                         # Nx, Ny, Nz, Hx, Hy, Hz
PARENT = 56 * 48 * 208 * 8
BASE, FAR = 1 << 32, 1 << 42
FIELDS = [BASE + q * PARENT for q in range(17)]
KAPPA, SCRATCH = FAR, FAR + 4 * PARENT
DZC, DZF, COUNTS = 1 << 20, 2 << 20, 3 << 20
BOUND = "Nz = 200 is beyond the on-chip path's 160 levels (tpg_vertical_diffusion_on_chip_levels): pass scratch and TPG_VDIFF_STREAMED or TPG_VDIFF_AUTO"
WHY = " (an item writes its own cells while other items read theirs)"
CONSTANT, PROFILE, FIELD = 0, 1, 2
AUTO, ON_CHIP, STREAMED = 0, 1, 2


def _call(osg, fields=None, n=None, kappa=None, kappa_value=0.5, form=CONSTANT, dz_c=DZC, dz_f=DZF, counts=COUNTS, dt=0.7, scratch=None,
          path=ON_CHIP, geom=G, ft=1, table=True):
    L = osg._lib
    fields = FIELDS[:3] if fields is None else fields
    ptrs = (L.C.c_void_p * len(fields))(*fields) if table else None
    return L.vertical_diffusion_lib().tpg_vertical_implicit_diffusion(ptrs, len(fields) if n is None else n, kappa, kappa_value, form, dz_c, dz_f,
                                                                      counts, 0.0, dt, scratch, path, *geom, ft, None)


def test_header_exports_and_signatures_are_the_three_names(osg):
    from test_abi import ROOT, declared_symbols, exported_symbols
    L = osg._lib
    L.vertical_diffusion_lib()
    assert sorted(declared_symbols("tripolar_hip_vertical_diffusion.h")) == NAMES == sorted(exported_symbols(L.VERTICAL_DIFFUSION_LIB_PATH)) \
        == sorted(L.VERTICAL_DIFFUSION_SIGNATURES)
    restype, argtypes = L.VERTICAL_DIFFUSION_SIGNATURES["tpg_vertical_implicit_diffusion"]
    assert len(argtypes) == 20 and [q for q, t in enumerate(argtypes) if t is L.C.c_double] == [3, 8, 9]


def test_on_chip_levels_is_monotone_in_n(osg):
    lib = osg._lib.vertical_diffusion_lib()
    for ft in (0, 1):
        levels = [lib.tpg_vertical_diffusion_on_chip_levels(n, ft) for n in range(1, 17)]
        assert all(a >= b for a, b in zip(levels, levels[1:])) and levels[-1] >= 75, levels       # never more levels for more fields
    for n, ft in ((0, 1), (17, 1), (-1, 0)):
        assert lib.tpg_vertical_diffusion_on_chip_levels(n, ft) == -1
        assert lib.tpg_vertical_diffusion_last_error().decode() == f"{n} fields: 1 to TPG_MAX_FIELDS = 16 in one call"
    assert lib.tpg_vertical_diffusion_on_chip_levels(1, 7) == -1 and lib.tpg_vertical_diffusion_last_error().decode() == "unknown element type ft=7"


def test_argument_errors_without_device_work(osg):
    """the nine refusals of the header, in its order: each is reached only when everything before it passes"""
    lib = osg._lib.vertical_diffusion_lib()
    err = lambda: lib.tpg_vertical_diffusion_last_error().decode()       # noqa: E731
    call = lambda **kw: _call(osg, **kw)                                 # noqa: E731
    assert call() == -5 and err() == BOUND                         # the base call passes the first seven checks
    # 1. the geometry (before the fields)
    assert call(ft=7, n=0) == -1 and err() == "unknown element type ft=7"
    assert call(geom=(49, 40, 3, 4, 4, 4)) == -2
    assert call(geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert call(geom=(48, 40, 3, 4, 4, -1)) == -1 and err().startswith("invalid size")
    # 2. the fields (before the form)
    assert call(n=0, form=9) == -1 and err() == "no fields"
    assert call(n=-3) == -1 and err() == "no fields"
    assert call(table=False) == -1 and err() == "no fields"
    assert call(fields=FIELDS, form=9) == -1 and err() == "17 fields: at most TPG_MAX_FIELDS = 16 in one call"
    for q in range(3):
        fields = list(FIELDS[:3])
        fields[q] = None
        assert call(fields=fields, path=9) == -1 and err() == f"null field {q}"
    assert call(fields=FIELDS[:16]) == -5 and err() == BOUND       # sixteen are served
    # 3. the form, then the path (before the pointers)
    for form in (3, -1, 7):
        assert call(form=form, path=9, dz_c=None) == -5 and err().startswith(f"kappa form {form} is not built (TPG_KAPPA_CONSTANT = 0")
    for path in (3, -1):
        assert call(path=path, dz_c=None) == -5 and err().startswith(f"path {path} is not built (TPG_VDIFF_AUTO = 0")
    # 4. the null combinations, in this order
    assert call(kappa=KAPPA, dz_c=None) == -1 and err() == "kappa given with TPG_KAPPA_CONSTANT: the diffusivity is kappa_value"
    assert call(form=PROFILE, dz_f=None) == -1 and err() == "null kappa with TPG_KAPPA_PROFILE"
    assert call(form=FIELD, path=STREAMED) == -1 and err() == "null kappa with TPG_KAPPA_FIELD"
    for name in ("dz_c", "dz_f"):
        assert call(path=STREAMED, **{name: None}) == -1 and err() == "null dz_c or dz_f"
    assert call(path=STREAMED, dt=math.nan) == -1 and err() == "TPG_VDIFF_STREAMED without scratch"
    # 5. the step and the constant (before alignment)
    for dt in (math.nan, math.inf, -math.inf):
        assert call(dt=dt, kappa_value=math.nan, dz_c=DZC + 4) == -1 and err() == "dt is not finite"
    for value in (math.nan, math.inf):
        assert call(kappa_value=value, dz_c=DZC + 4) == -1 and err() == "kappa_value is not finite"
        assert call(kappa_value=value, form=PROFILE, kappa=KAPPA) == -5 and err() == BOUND       # not read in the other forms
    # 6. alignment: to the element type, Float64 and Float32, and the counts to int32
    for q in range(3):
        for ft, off in ((1, 4), (0, 2)):
            fields = list(FIELDS[:3])
            fields[q] += off
            assert call(fields=fields, ft=ft, dz_c=DZC + off) == -1 and err() == f"field {q}: pointer not aligned to its element type"
    for kw in (dict(dz_c=DZC + 4), dict(dz_f=DZF + 4), dict(scratch=SCRATCH + 4), dict(kappa=KAPPA + 4, form=PROFILE), dict(kappa=KAPPA + 4, form=FIELD)):
        assert call(counts=COUNTS + 2, **kw) == -1 and err() == "kappa, dz_c, dz_f or scratch pointer not aligned to its element type"
    assert call(counts=COUNTS + 2, fields=[BASE, BASE + 8]) == -1 and err() == "count plane pointer not aligned to int32"
    # 7. the overlaps: identical, one element inside from either side; right behind or right in front is none
    for shift, status in ((0, -1), (8, -1), (-8, -1), (PARENT - 8, -1), (8 - PARENT, -1), (PARENT, -5), (-PARENT, -5)):
        at = FIELDS[8] + shift
        assert call(fields=[FIELDS[8], FIELDS[2], at]) == status and err() == ("field 0 overlaps field 2" + WHY if status == -1 else BOUND), shift
        assert call(fields=[FIELDS[2], FIELDS[8]], scratch=at) == status and err() == ("field 1 overlaps scratch" + WHY if status == -1 else BOUND), shift
        assert call(fields=[FIELDS[8]], form=FIELD, kappa=at) == status and err() == ("field 0 overlaps kappa" + WHY if status == -1 else BOUND), shift
        assert call(form=FIELD, kappa=KAPPA, scratch=KAPPA + shift) == status and err() == ("scratch overlaps kappa" + WHY if status == -1 else BOUND), shift
    table = 201 * 8                                                # a profile is Nz + 1 values
    for shift, status in ((0, -1), (table - 8, -1), (table, -5), (8 - PARENT, -1), (-PARENT, -5)):
        assert call(form=PROFILE, kappa=KAPPA, scratch=KAPPA + shift) == status and err() == ("scratch overlaps kappa" + WHY if status == -1 else BOUND), shift
    assert call(form=PROFILE, kappa=FIELDS[1] + 16) == -5 and err() == BOUND                    # a profile is not checked against the fields
    # 8. the on-chip bound: on the on-chip path, and on AUTO without scratch; the message states the bound
    assert lib.tpg_vertical_diffusion_on_chip_levels(3, 1) == 160
    assert call(path=AUTO) == -5 and err() == BOUND
    assert call(geom=(48, 40, 161, 4, 4, 4)) == -5 and err().startswith("Nz = 161 is beyond the on-chip path's 160 levels")
    assert call(geom=(2, 1, 161, 1, 1, 1), fields=[BASE]) == -5 and err().startswith("Nz = 161")          # the smallest plane passes the geometry
    assert call(geom=(48, 40, 200, 0, 0, 0)) == -5 and err() == BOUND                                     # every halo width down to 0 is admitted
    # 9. more work items than 32 bits index: refused by the plane check every entry point shares
    assert call(geom=(65536, 32768, 1, 1, 1, 1), ft=0, fields=[1 << 44, 2 << 44], counts=None) == -5 and "32-bit" in err()


def test_the_records_and_the_closures_refused_by_name(osg):
    from orthogonalsphericalshellgrids.jl_amd import vertical_diffusion as vd
    implicit, explicit = osg.VerticallyImplicitTimeDiscretization(), osg.ExplicitTimeDiscretization()
    c = osg.VerticalScalarDiffusivity(implicit, nu=1e-2, kappa=1e-4)
    assert c == osg.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4) and c.time_discretization == implicit and implicit != explicit
    assert osg.VerticalScalarDiffusivity(implicit, 1e-2, {"T": 1e-4, "S": 2e-4}).kappa["S"] == 2e-4
    assert vd.refuse_closure(c, "x") is c
    with pytest.raises(NotImplementedError, match="x: ExplicitTimeDiscretization is not built: the explicit diffusive tendency is out of scope") as e:
        vd.refuse_closure(osg.VerticalScalarDiffusivity(explicit, 1e-2, 1e-4), "x")
    assert "VerticallyImplicitTimeDiscretization()" in str(e.value)
    for name in ("HorizontalScalarDiffusivity", "ConvectiveAdjustmentVerticalDiffusivity", "RiBasedVerticalDiffusivity", "CATKEVerticalDiffusivity",
                 "ScalarDiffusivity", "IsopycnalSkewSymmetricDiffusivity"):
        with pytest.raises(NotImplementedError, match=f"x: {name} is not built") as e:
            vd.refuse_closure(type(name, (), {})(), "x")
        assert "VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), nu, kappa) is built" in str(e.value)
        assert "a diffusivity computed by the host can be passed as a Field" in str(e.value)
    with pytest.raises(NotImplementedError, match="closure None is not built"):
        vd.refuse_closure(None, "x")
    with pytest.raises(NotImplementedError, match="is a time discretization, not a closure"):
        vd.refuse_closure(implicit, "x")


def test_python_refusals_and_plans_on_host_grids(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd._operator_plan import OperatorPlan
    for name in ("vertical_implicit_diffusion", "vertical_implicit_diffusion_plan", "VerticalImplicitDiffusionPlan", "implicit_step_plan",
                 "ImplicitStepPlan", "VerticalScalarDiffusivity", "VerticallyImplicitTimeDiscretization", "ExplicitTimeDiscretization"):
        assert hasattr(osg, name), name
    for name in ("vertical_diffusion_lib", "check_vertical_diffusion", "VERTICAL_DIFFUSION_SIGNATURES", "VERTICAL_DIFFUSION_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    assert issubclass(osg.VerticalImplicitDiffusionPlan, OperatorPlan)
    grid, other = _grid(osg), _grid(osg)
    u, v, c, d = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid), osg.CenterField(grid)
    w = osg.ZFaceField(grid)
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))       # noqa: E731
    window = (slice(None), slice(None), range(1, 3))
    plan_of = osg.vertical_implicit_diffusion_plan
    for fn in (plan_of, osg.vertical_implicit_diffusion):
        with pytest.raises(TypeError, match="no fields"):
            fn([], 1.0, 0.5)
        with pytest.raises(TypeError, match="field 1 must be a Field"):
            fn([c, c.data], 1.0, 0.5)
        with pytest.raises(TypeError, match=r"the fields must be Center in z .* \(field 0 at \(Center, Center, Face\)\)"):
            fn(w, 1.0, 0.5)
        with pytest.raises(ValueError, match=r"share one matrix, so one location: field 1 at \(Face, Center, Center\) against \(Center, Center, Center\)"):
            fn([c, u], 1.0, 0.5)
        with pytest.raises(ValueError, match="one grid"):
            fn([c, osg.CenterField(other)], 1.0, 0.5)
        with pytest.raises(ValueError, match="one element type"):
            fn([c, f32(osg.CenterField)], 1.0, 0.5)
        with pytest.raises(NotImplementedError, match="z-windowed"):
            fn([c, osg.CenterField(grid, indices=window)], 1.0, 0.5)
        with pytest.raises(ValueError, match="field 1 is field 0 itself"):
            fn([c, osg.CenterField(grid, data=c.data)], 1.0, 0.5)
        with pytest.raises(ValueError, match="path 'lds' is not one of 'auto', 'on_chip' and 'streamed'"):
            fn(c, 1.0, 0.5, path="lds")
        # kappa: a Field at the fields' horizontal location and Face in z, a profile of Nz + 1 values of the fields' type, a number
        with pytest.raises(TypeError, match=r"a kappa Field must be at \(Face, Center, Face\).*\(it is at \(Center, Center, Face\)\): interpolating"):
            fn(u, w, 0.5)
        with pytest.raises(TypeError, match=r"a kappa Field must be at \(Center, Center, Face\)"):
            fn(c, d, 0.5)
        with pytest.raises(ValueError, match="one grid"):
            fn(c, osg.ZFaceField(other), 0.5)
        with pytest.raises(ValueError, match=r"a kappa profile must be a contiguous tensor of Nz \+ 1 = 4 face values"):
            fn(c, torch.zeros(3, dtype=torch.float64), 0.5)
        with pytest.raises(ValueError, match="a kappa profile must be"):
            fn(c, torch.zeros(4, dtype=torch.float32), 0.5)
        with pytest.raises(TypeError, match="kappa must be a number, a tensor of Nz \\+ 1 face values or a Field"):
            fn(c, "much", 0.5)
    # the plans on a host-only record: built, never called
    p = plan_of([c, d], 0.25, 0.5)
    assert p.dt == 0.5 and p.scratch is not None and p._call[1][10] == p.scratch.data_ptr() and p._call[1][1] == 2 and p._call[1][3:5] == (0.25, 0) and p._call[1][9] == 0.5 and p._call[1][11] == 0
    q = p.with_dt(0.125)
    assert q.dt == 0.125 and q._call[1][9] == 0.125 and p._call[1][9] == 0.5 and q._call[1][:9] == p._call[1][:9] and q.fields is p.fields
    s = plan_of(c, torch.ones(4, dtype=torch.float64), 0.5, path="streamed")
    assert s.scratch is not None and s.scratch.shape == c.data.shape and s._call[1][4] == 1 and s._call[1][11] == 2
    assert s._call[1][10] == s.scratch.data_ptr() and s.with_dt(1.0).scratch is s.scratch
    k = plan_of(u, osg.Field((osg.Face, osg.Center, osg.Face), grid), 0.5, path="on_chip")
    assert k._call[1][4] == 2 and k._call[1][11] == 1 and k._call[1][7] is None                            # no count plane on a bare grid
    assert k.scratch is None and k._call[1][10] is None and plan_of(d, 0.25, 0.5, scratch=s.scratch).scratch is s.scratch
    with pytest.raises(ValueError, match="scratch must be a contiguous tensor of the fields' parent shape"):
        plan_of(d, 0.25, 0.5, scratch=torch.zeros(3))
    many = [osg.CenterField(grid) for _ in range(35)]                                                      # more than 16 fields: three calls
    m = plan_of(many, 0.25, 0.5)
    assert [b._call[1][1] for b in m._before] + [m._call[1][1]] == [16, 16, 3]
    assert [b._call[1][9] for b in m.with_dt(2.0)._before] == [2.0, 2.0]
    # the model's implicit step
    closure = osg.VerticalScalarDiffusivity(osg.VerticallyImplicitTimeDiscretization(), nu=1e-2, kappa={"T": 1e-4, "S": 1e-4, "e": 3e-4})
    step = osg.implicit_step_plan(u, v, {"T": c, "S": d, "e": many[0]}, closure, 0.5)
    assert [len(x.fields) for x in step.plans] == [1, 1, 2, 1] and [x._call[1][3] for x in step.plans] == [1e-2, 1e-2, 1e-4, 3e-4]
    assert step.plans[0].fields == [u] and step.plans[2].fields == [c, d] and all(x.scratch is step.plans[0].scratch for x in step.plans)
    assert [x.dt for x in step.with_dt(0.25).plans] == [0.25] * 4 and step.dt == 0.5
    one = osg.implicit_step_plan(None, None, [c, d], osg.VerticalScalarDiffusivity(nu=0.0, kappa=2e-4), 0.5)
    assert len(one.plans) == 1 and one.plans[0]._call[1][1] == 2
    with pytest.raises(NotImplementedError, match="implicit_step_plan: CATKEVerticalDiffusivity is not built"):
        osg.implicit_step_plan(u, v, [c], type("CATKEVerticalDiffusivity", (), {})(), 0.5)
    with pytest.raises(NotImplementedError, match="ExplicitTimeDiscretization is not built"):
        osg.implicit_step_plan(u, v, [c], osg.VerticalScalarDiffusivity(osg.ExplicitTimeDiscretization(), 1.0, 1.0), 0.5)
    with pytest.raises(TypeError, match="a per-tracer kappa needs the tracers as a mapping"):
        osg.implicit_step_plan(u, v, [c], closure, 0.5)
    with pytest.raises(KeyError, match="no entry for the tracers"):
        osg.implicit_step_plan(u, v, {"b": c}, closure, 0.5)
    with pytest.raises(TypeError, match="no fields"):
        osg.implicit_step_plan(None, None, [], osg.VerticalScalarDiffusivity(nu=0.0, kappa=2e-4), 0.5)


def test_missing_library_fails_loudly(osg, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the plan raises: it computes nothing some other way"""
    missing = str(tmp_path / os.path.basename(osg._lib.VERTICAL_DIFFUSION_LIB_PATH))
    monkeypatch.setattr(osg._lib, "_vertical_diffusion", None)
    monkeypatch.setattr(osg._lib, "VERTICAL_DIFFUSION_LIB_PATH", missing)
    with pytest.raises(ImportError, match="only backend"):
        osg.vertical_implicit_diffusion_plan(osg.CenterField(_grid(osg)), 1.0, 0.5)


def test_the_build_names_the_library_the_map_and_its_records():
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "-ffp-contract=off" in make
    text = open(os.path.join(csrc, "vertical_diffusion.map")).read()
    assert all(n in text for n in NAMES) and "local: *;" in text
    body = open(os.path.join(csrc, "tpg_vertical_diffusion.hip")).read()
    assert '#include "tpg_operator.hpp"' in body and "check_overlaps(" in body and "chunk_plan<T>" in body and "getenv" not in body
    assert body.count("__global__") == 1 and "__syncthreads" not in body and "atomic" not in body.replace("No atomics", "") and "hipMalloc" not in body
    # the record of the build: nothing differs in an existing object; nothing in private memory, no static LDS, no vector-register spill
    diff = json.load(open(os.path.join(ROOT, "profiles", "vertical_diffusion", "isa_diff.json")))
    assert "tpg_hydrostatic.o" in diff and "tpg_timestep.o" in diff and "tpg_grid.o" in diff and len(diff) >= 26
    for name, r in diff.items():
        assert not any(r.get(k) for k in ("differing", "metadata_differing", "only_old", "only_new", "renamed")), name
    res = json.load(open(os.path.join(ROOT, "profiles", "vertical_diffusion", "resources.json")))["kernels"]
    assert len(res) == 80 and all("k_vertical_implicit_diffusion" in k for k in res)       # 5 chunk forms x FIELD or not x 2 policies x 4 field bounds
    for k, r in res.items():
        assert (r["vgpr_spill_count"], r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["uses_dynamic_stack"]) == ("0", "0", "0", "false"), k
        assert int(r["vgpr_count"]) <= 512 and int(r["max_flat_workgroup_size"]) in (64, 256), k
