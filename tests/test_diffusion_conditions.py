"""Host-side tests of the explicit diffusive tendency (no GPU): the export list of libtripolar_hip_diffusion.so, which is staged beside the
table of the libraries; every argument error of tpg_diffusive_tendency in the order its header gives (status and message; every call below
fails in validation, none reaches a launch, the pointers are fabricated and never dereferenced: a call that passes a check is refused by a
later one, at the latest by the stencil check, the ninth, at halo (0, 0, 0)); every refusal and record of the Python layer on host-only grid
records; the loader; and that the table itself is as the parent left it."""
import difflib
import math
import os
import re
import subprocess

import pytest

from test_abi import ROOT, exported_symbols
from test_weno_momentum_conditions import _grid

CSRC = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
STAGED = os.path.join(CSRC, "staged")
NAMES = ["tpg_diffusion_last_error", "tpg_diffusive_tendency"]
CONSTANTS = {"TPG_DIFFUSION_HORIZONTAL": 1, "TPG_DIFFUSION_VERTICAL": 2, "TPG_DIFFUSION_ADD": 0, "TPG_DIFFUSION_WRITE": 1,
             "TPG_DIFFUSION_KAPPA_CONSTANT": 0, "TPG_DIFFUSION_KAPPA_PROFILE": 1, "TPG_DIFFUSION_KAPPA_FIELD": 2}
G0 = (48, 40, 6, 0, 0, 0)                                          # Nx, Ny, Nz at halo (0, 0, 0): the stencil check refuses what passes the rest
PARENT, PLANE = 48 * 40 * 6 * 8, 48 * 40 * 8
BASE = 1 << 32
FIELDS = [BASE + 4 * q * PARENT for q in range(17)]               # four parents apart: room for the halos of the stencil cases
OUTS = [BASE + 4 * (32 + q) * PARENT for q in range(17)]
FAR = 1 << 42
KAPPA, H, ZC, COUNTS = FAR, FAR + 8 * PARENT, 5 << 20, 6 << 20
DXF, DYF, DXC, DYC, AZ, DZC, DZF = (7 + q << 20 for q in range(7))
TOPS = [FAR + (16 + q) * PARENT for q in range(3)]
BOTS = [FAR + (24 + q) * PARENT for q in range(3)]
HORIZONTAL, VERTICAL = 1, 2
ADD, WRITE = 0, 1
CONSTANT, PROFILE, FIELD = 0, 1, 2
# the lines `make -n -B -C csrc HIPCC=hipcc ARCH=gfx950` printed (without make's own "Entering directory" lines) on the commit this library was
# staged on: the two variables are given on the command line, so nothing of the environment enters the text
PARENT_MAKE = os.path.join(ROOT, "tests", "golden", "diffusion", "make_n_B_csrc.txt")
STENCIL = ("the rule reads c[i-1..i+1, j, k], c[i, j-1..j+1, k] and the same cells of bottom_height: Hx >= 1 and Hy >= 1 needed with "
           "TPG_DIFFUSION_HORIZONTAL (halo (0,0,0))")


def _header():
    text = open(os.path.join(STAGED, "tripolar_hip_diffusion.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _call(osg, c=None, G=None, n=None, terms=HORIZONTAL | VERTICAL, mode=ADD, kappa_h=0.5, kappa_z=None, kappa_z_value=0.25, form=CONSTANT,
          top=None, bottom=None, dx_fc=DXF, dy_fc=DYF, dx_cf=DXC, dy_cf=DYC, az=AZ, dz_c=DZC, dz_f=DZF, counts=COUNTS, h=H, zc=ZC, wall=1, geom=G0,
          ft=1, tables=(True, True)):
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    L = osg._lib
    c = FIELDS[:3] if c is None else c
    G = OUTS[:len(c)] if G is None else G
    table = lambda a: None if a is None else (L.C.c_void_p * len(a))(*a)          # noqa: E731
    return D.diffusion_lib().tpg_diffusive_tendency(table(c) if tables[0] else None, table(G) if tables[1] else None, len(c) if n is None else n,
                                                    terms, mode, kappa_h, kappa_z, kappa_z_value, form, table(top), table(bottom), dx_fc, dy_fc,
                                                    dx_cf, dy_cf, az, dz_c, dz_f, counts, 0.0, h, zc, wall, *geom, ft, None)


def test_header_map_exports_and_signatures_are_the_two_names(osg):
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    D.diffusion_lib()
    _, code = _header()
    declared = sorted(set(re.findall(r"\b(tpg_[a-z0-9_]+)\s*\(", code)))
    text = open(os.path.join(STAGED, "diffusion.map")).read()
    assert "local: *;" in text
    assert declared == NAMES == sorted(re.findall(r"\btpg_[a-z0-9_]+", text)) == sorted(exported_symbols(D.DIFFUSION_LIB_PATH)) == sorted(D.DIFFUSION_SIGNATURES)
    restype, argtypes = D.DIFFUSION_SIGNATURES["tpg_diffusive_tendency"]
    assert len(argtypes) == 31 and [q for q, t in enumerate(argtypes) if t is osg._lib.C.c_double] == [5, 7, 19]
    for other in osg._lib.LIBRARIES:                               # no name of it is in a library of the table
        path = getattr(osg._lib, osg._lib.LIBRARIES[other].path_global)
        assert not set(NAMES) & set(exported_symbols(path)), other


def test_library_reads_no_environment_variable():
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    D.diffusion_lib()
    und = subprocess.run(["nm", "-D", "--undefined-only", D.DIFFUSION_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und


def test_header_is_plain_c_with_its_seven_constants(tmp_path):
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    src = tmp_path / "abi.c"
    src.write_text('#include "tripolar_hip_diffusion.h"\ntypedef void (*fn)(void);\nstatic fn table[] = {' + ", ".join(f"(fn){n}" for n in NAMES)
                   + "};\n" + "".join(f"typedef char value_of_{c}[({c} == {v}) ? 1 : -1];\n" for c, v in CONSTANTS.items())
                   + "int main(void) { return sizeof(table) == 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", STAGED, "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for constant, value in CONSTANTS.items():
        assert getattr(D, constant) == value, constant
    defined = re.findall(r"#define (TPG_[A-Z0-9_]+) ", _header()[0])
    assert sorted(c for c in defined if not c.endswith("_H")) == sorted(CONSTANTS)


def test_missing_library_fails_loudly(osg, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the binding and the plan raise, and name the path they looked at"""
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    missing = str(tmp_path / os.path.basename(D.DIFFUSION_LIB_PATH))
    monkeypatch.setattr(D, "_diffusion", None)
    monkeypatch.setattr(D, "DIFFUSION_LIB_PATH", missing)
    with pytest.raises(ImportError, match="only backend") as err:
        D.diffusion_lib()
    assert missing in str(err.value)
    grid = _grid(osg)
    with pytest.raises(ImportError, match="only backend"):
        osg.diffusive_tendency_plan(osg.CenterField(grid), osg.CenterField(grid), horizontal=1.0)


def test_argument_errors_without_device_work(osg):
    """the ten refusals of the header, in its order: each is reached only when everything before it passes"""
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    lib = D.diffusion_lib()
    err = lambda: lib.tpg_diffusion_last_error().decode()         # noqa: E731
    call = lambda **kw: _call(osg, **kw)                           # noqa: E731
    assert call() == -5 and err() == STENCIL                       # the base call passes the first eight checks
    # 1. the geometry (before the fields)
    assert call(ft=7, n=0) == -1 and err() == "unknown element type ft=7"
    assert call(geom=(49, 40, 3, 4, 4, 4)) == -2
    assert call(geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert call(geom=(48, 4, 3, 4, 5, 4)) == -5 and err().startswith("halo (4,5) larger than size")
    # 2. the fields (before the terms)
    assert call(n=0, terms=8) == -1 and err() == "no fields (nfields = 0)"
    assert call(n=-3) == -1 and err() == "no fields (nfields = -3)"
    assert call(c=FIELDS, G=OUTS, terms=8) == -1 and err() == "17 fields: at most TPG_MAX_FIELDS = 16 in one call"
    for tables in ((False, True), (True, False)):
        assert call(tables=tables, terms=8) == -1 and err() == "null table of fields or of tendencies"
    for q in range(3):
        c, G = list(FIELDS[:3]), list(OUTS[:3])
        c[q] = None
        assert call(c=c, terms=8) == -1 and err() == f"null field {q}"
        G[q] = None
        assert call(G=G, terms=8) == -1 and err() == f"null G of field {q}"
    assert call(c=FIELDS[:16], G=OUTS[:16]) == -5 and err() == STENCIL            # sixteen are served
    # 3. the groups (before the mode)
    for terms in (4, 7, -1, 1 << 20):
        assert call(terms=terms, mode=9) == -5 and err() == f"terms {terms} has bits that are not built (TPG_DIFFUSION_HORIZONTAL = 1 and TPG_DIFFUSION_VERTICAL = 2 are)"
    assert call(terms=0, mode=9) == -1 and err() == "no group is present: terms = 0 and no table of top or bottom fluxes"
    assert call(terms=0, mode=9, top=[None] * 3) == -5 and err().startswith("mode 9")       # a table makes the vertical group present
    assert call(terms=0, mode=9, bottom=BOTS) == -5 and err().startswith("mode 9")
    # 4. the mode, then the form (before the pointers)
    for mode in (2, -1):
        assert call(mode=mode, form=9, az=None) == -5 and err() == f"mode {mode} is not built (TPG_DIFFUSION_ADD = 0 and TPG_DIFFUSION_WRITE = 1 are)"
    for form in (3, -1, 7):
        assert call(form=form, az=None) == -5 and err().startswith(f"kappa_z form {form} is not built (TPG_DIFFUSION_KAPPA_CONSTANT = 0")
    # 5. the null combinations, in this order
    assert call(kappa_z=KAPPA, az=None) == -1 and err() == "kappa_z given with TPG_DIFFUSION_KAPPA_CONSTANT: the diffusivity is kappa_z_value"
    assert call(form=PROFILE, az=None) == -1 and err() == "null kappa_z with TPG_DIFFUSION_KAPPA_PROFILE"
    assert call(form=FIELD, az=None) == -1 and err() == "null kappa_z with TPG_DIFFUSION_KAPPA_FIELD"
    for name in ("dz_c", "az"):
        assert call(dz_f=None, **{name: None}) == -1 and err() == "null dz_c or az"
    assert call(dz_f=None, dx_fc=None) == -1 and err() == "null dz_f with TPG_DIFFUSION_VERTICAL"
    assert call(dz_f=None, terms=HORIZONTAL) == -5 and err() == STENCIL           # not read without the interior faces
    assert call(dz_f=None, terms=HORIZONTAL, top=TOPS) == -5 and err() == STENCIL
    for name in ("dx_fc", "dy_fc", "dx_cf", "dy_cf"):
        assert call(zc=None, **{name: None}) == -1 and err() == "null dx_fc, dy_fc, dx_cf or dy_cf with TPG_DIFFUSION_HORIZONTAL"
    assert call(zc=None, kappa_h=math.nan) == -1 and err() == "bottom_height without z_centers"
    assert call(h=None, zc=None) == -5 and err() == STENCIL        # no closed faces: the older convention
    # a vertical-only call reads no horizontal metric and takes every halo width: it passes every check, so its launch would follow --
    # it is made with a table overlap instead
    assert call(terms=VERTICAL, dx_fc=None, dy_fc=None, dx_cf=None, dy_cf=None, G=[FIELDS[0]] + OUTS[1:3]) == -1 and err().startswith("G of field 0 overlaps field 0")
    # 6. the numbers (before alignment)
    for value in (math.nan, math.inf, -math.inf):
        assert call(kappa_h=value, kappa_z_value=math.nan, az=AZ + 4) == -1 and err() == "kappa_h is not finite"
        assert call(kappa_z_value=value, az=AZ + 4) == -1 and err() == "kappa_z_value is not finite"
        assert call(kappa_z_value=value, form=PROFILE, kappa_z=KAPPA) == -5 and err() == STENCIL              # not read in the other forms
        assert call(kappa_z_value=value, terms=HORIZONTAL) == -5 and err() == STENCIL
        assert call(kappa_h=value, terms=VERTICAL, c=[FIELDS[0]], G=[FIELDS[0]]) == -1 and err().startswith("G of field 0 overlaps")
    # 7. alignment: to the element type, Float64 and Float32, and the counts to int32
    for q in range(3):
        for ft, off in ((1, 4), (0, 2)):
            c, G = list(FIELDS[:3]), list(OUTS[:3])
            c[q] += off
            assert call(c=c, ft=ft, az=AZ + off) == -1 and err() == f"field {q}: pointer not aligned to its element type"
            G[q] += off
            assert call(G=G, ft=ft, az=AZ + off) == -1 and err() == f"G of field {q}: pointer not aligned to its element type"
            for side in ("top", "bottom"):
                planes = [None] * 3
                planes[q] = TOPS[q] + off
                assert call(ft=ft, az=AZ + off, **{side: planes}) == -1 and err() == f"flux plane of field {q}: pointer not aligned to its element type"
    shared = "kappa_z, a metric plane, dz_c, dz_f, bottom_height or z_centers pointer not aligned to its element type"
    for kw in (dict(dx_fc=DXF + 4), dict(dy_fc=DYF + 4), dict(dx_cf=DXC + 4), dict(dy_cf=DYC + 4), dict(az=AZ + 4), dict(dz_c=DZC + 4), dict(dz_f=DZF + 4),
               dict(h=H + 4), dict(zc=ZC + 4), dict(kappa_z=KAPPA + 4, form=PROFILE), dict(kappa_z=KAPPA + 4, form=FIELD)):
        assert call(counts=COUNTS + 2, **kw) == -1 and err() == shared, kw
    assert call(counts=COUNTS + 2, G=[FIELDS[0]] + OUTS[1:3]) == -1 and err() == "count plane pointer not aligned to int32"
    # 8. the overlaps: identical, one element inside from either side; right behind or right in front is none
    why = " (every item reads cells while its neighbours write: not an in-place call)"
    for shift, status in ((0, -1), (8, -1), (-8, -1), (PARENT - 8, -1), (8 - PARENT, -1), (PARENT, -5), (-PARENT, -5)):
        at = OUTS[8] + shift
        hit = status == -1
        assert call(c=[FIELDS[0], at, FIELDS[2]], G=[OUTS[0], OUTS[1], OUTS[8]]) == status and err() == ("G of field 2 overlaps field 1" + why if hit else STENCIL), shift
        assert call(G=[OUTS[8], OUTS[1], at]) == status and err() == ("G of field 2 overlaps G of field 0" if hit else STENCIL), shift
        assert call(G=[OUTS[0], OUTS[8], OUTS[2]], form=PROFILE, kappa_z=at) == -5 and err() == STENCIL                # a profile is not checked
    field_kappa = 48 * 40 * 7 * 8                                  # a FIELD kappa has one more level
    for shift, status in ((0, -1), (PARENT - 8, -1), (8 - field_kappa, -1), (PARENT, -5), (-field_kappa, -5)):
        assert call(G=[OUTS[8]], c=[FIELDS[0]], form=FIELD, kappa_z=OUTS[8] + shift) == status and err() == ("G of field 0 overlaps kappa_z" if status == -1 else STENCIL), shift
    for shift, status in ((0, -1), (PARENT - 8, -1), (8 - PLANE, -1), (PARENT, -5), (-PLANE, -5)):
        at = OUTS[8] + shift
        hit = status == -1
        two = dict(c=FIELDS[:2], G=[OUTS[0], OUTS[8]])
        assert call(top=[at, None], **two) == status and err() == ("G of field 1 overlaps the top flux plane of field 0" if hit else STENCIL), shift
        assert call(bottom=[None, at], **two) == status and err() == ("G of field 1 overlaps the bottom flux plane of field 1" if hit else STENCIL), shift
        assert call(h=at, **two) == status and err() == ("G of field 1 overlaps bottom_height" if hit else STENCIL), shift
    # 9. the stencil: the horizontal group with Hx < 1 or Hy < 1
    for halo in ((0, 1, 1), (1, 0, 1), (0, 0, 4)):
        assert call(geom=(48, 40, 6, *halo)) == -5 and err() == STENCIL.replace("(0,0,0)", "(%d,%d,%d)" % halo)
    # 10. more work items than 32 bits index: the plane check every entry point shares refuses every such geometry first (a plane below 2^31
    # cells has fewer than 2^30 work items), as the header says: the tenth message cannot be reached, and this is the first check's
    assert call(geom=(65536, 32768, 1, 1, 1, 1), ft=0, c=[1 << 44], G=[2 << 44], counts=None) == -5 and "32-bit" in err()


def test_the_record_and_the_closures_refused_by_name(osg):
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    assert osg.HorizontalScalarDiffusivity() == osg.HorizontalScalarDiffusivity(nu=0.0, kappa=0.0)
    assert osg.HorizontalScalarDiffusivity(kappa=2.5).kappa == 2.5
    grid = _grid(osg)
    c, G = osg.CenterField(grid), osg.CenterField(grid)
    plan_of = osg.diffusive_tendency_plan
    with pytest.raises(NotImplementedError, match=r"HorizontalScalarDiffusivity\(nu=0.1\): horizontal viscosity in Oceananigans' divergence-vorticity form is not built") as e:
        plan_of(c, G, horizontal=osg.HorizontalScalarDiffusivity(nu=0.1, kappa=1.0))
    assert D.BUILT in str(e.value) and "HorizontalScalarDiffusivity(kappa=number)" in D.BUILT and "ExplicitTimeDiscretization()" in D.BUILT
    for name in ("ConvectiveAdjustmentVerticalDiffusivity", "RiBasedVerticalDiffusivity", "CATKEVerticalDiffusivity", "ScalarDiffusivity",
                 "IsopycnalSkewSymmetricDiffusivity", "HorizontalScalarBiharmonicDiffusivity"):
        with pytest.raises(NotImplementedError, match=f"{name} is not built") as e:
            plan_of(c, G, vertical=type(name, (), {})())
        assert D.BUILT in str(e.value)
        with pytest.raises(NotImplementedError, match=f"{name} is not built as a horizontal closure") as e:
            plan_of(c, G, horizontal=type(name, (), {})())
        assert D.BUILT in str(e.value)
    with pytest.raises(NotImplementedError, match="VerticallyImplicitTimeDiscretization is the implicit step's"):
        plan_of(c, G, vertical=osg.VerticalScalarDiffusivity(osg.VerticallyImplicitTimeDiscretization(), 1.0, 1.0))
    with pytest.raises(NotImplementedError, match="ExplicitTimeDiscretization is a time discretization, not a closure"):
        plan_of(c, G, vertical=osg.ExplicitTimeDiscretization())
    with pytest.raises(NotImplementedError, match="a horizontal diffusivity .* is not built: kappa_h is one number"):
        plan_of(c, G, horizontal=osg.HorizontalScalarDiffusivity(kappa={"T": 1.0}))
    with pytest.raises(TypeError, match="share one kappa_z"):
        plan_of(c, G, vertical=osg.VerticalScalarDiffusivity(osg.ExplicitTimeDiscretization(), 1.0, {"T": 1.0}))


def test_python_refusals_and_plans_on_host_grids(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    from orthogonalsphericalshellgrids.jl_amd._operator_plan import OperatorPlan
    for name in ("diffusive_tendency", "diffusive_tendency_plan", "DiffusiveTendencyPlan", "HorizontalScalarDiffusivity"):
        assert hasattr(osg, name), name
    assert issubclass(osg.DiffusiveTendencyPlan, OperatorPlan)
    metrics = lambda: {k: torch.ones(6 + 2 * 3, 8 + 2 * 3, dtype=torch.float64) for k in ('lambda_cc', 'dx_fc', 'dy_fc', 'dx_cf', 'dy_cf', 'az_cc', 'az_fc')}       # noqa: E731
    grid, other = _grid(osg, arrays=metrics()), _grid(osg, arrays=metrics())
    u, v, c, d, G, H_ = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid), osg.CenterField(grid), osg.CenterField(grid), osg.CenterField(grid)
    Gu = osg.XFaceField(grid)
    w = osg.ZFaceField(grid)
    explicit = osg.VerticalScalarDiffusivity(osg.ExplicitTimeDiscretization(), nu=1e-2, kappa=1e-4)
    plan_of = osg.diffusive_tendency_plan
    for fn in (plan_of, osg.diffusive_tendency):
        with pytest.raises(TypeError, match="no fields"):
            fn([], [], horizontal=1.0)
        with pytest.raises(TypeError, match=r"fields and G are lists of one length \(2, 1\)"):
            fn([c, d], [G], horizontal=1.0)
        with pytest.raises(TypeError, match="field 1 must be a Field"):
            fn([c, c.data], [G, H_], horizontal=1.0)
        with pytest.raises(TypeError, match=r"the fields must be Center in z .* \(field 0 at \(Center, Center, Face\)\)"):
            fn(w, osg.ZFaceField(grid), vertical=1.0)
        with pytest.raises(ValueError, match=r"one location: field 1 at \(Face, Center, Center\) against \(Center, Center, Center\)"):
            fn([c, u], [G, Gu], vertical=1.0)
        with pytest.raises(TypeError, match=r"G of field 0 must be a Field at \(Face, Center, Center\)"):
            fn(u, G, vertical=1.0)
        with pytest.raises(ValueError, match="mode 'subtract' is not one of 'add' and 'write'"):
            fn(c, G, horizontal=1.0, mode="subtract")
        with pytest.raises(NotImplementedError, match=r"the horizontal group is defined for fields at \(Center, Center, Center\) only \(they are at \(Face, Center, Center\)\)"):
            fn(u, Gu, horizontal=1.0)
        with pytest.raises(ValueError, match="one grid"):
            fn([c, osg.CenterField(other)], [G, H_], horizontal=1.0)
        with pytest.raises(ValueError, match="G of field 0 is field 0 itself"):
            fn(c, osg.CenterField(grid, data=c.data), horizontal=1.0)
        with pytest.raises(ValueError, match="G of field 1 and G of field 0 are one field"):
            fn([c, d], [G, osg.CenterField(grid, data=G.data)], horizontal=1.0)
        with pytest.raises(TypeError, match=r"a kappa Field must be at \(Face, Center, Face\)"):
            fn(u, Gu, vertical=w)
        with pytest.raises(ValueError, match=r"a kappa profile must be a contiguous tensor of Nz \+ 1 = 4 face values"):
            fn(c, G, vertical=torch.zeros(3, dtype=torch.float64))
        with pytest.raises(TypeError, match="nothing to compute"):
            fn(c, G)
        with pytest.raises(ValueError, match="top_flux 'model' is not 'from_fields'"):
            fn(c, G, top_flux="model")
        with pytest.raises(TypeError, match=r"bottom_flux is a list of one entry per field \(1 for 2 fields\)"):
            fn([c, d], [G, H_], bottom_flux=[1.0])
        with pytest.raises(ValueError, match=r"a top flux must be None, a number, a contiguous \(\d+, \d+\) tensor"):
            fn(c, G, top_flux=torch.zeros(3, dtype=torch.float64))
        with pytest.raises(ValueError, match="a top flux Field must be a reduced Field"):
            fn(c, G, top_flux=d)
    # the plans on a host-only record: built, never called
    p = plan_of([c, d], [G, H_], horizontal=osg.HorizontalScalarDiffusivity(kappa=2.5), vertical=explicit)
    args = p._call[1]
    assert args[2:6] == (2, 3, 0, 2.5) and args[6] is None and args[7:9] == (1e-4, 0) and args[9] is None and args[10] is None
    assert all(a is not None for a in args[11:18]) and args[18] is None and args[20] is None and p.terms == 3        # no counts on a bare grid
    pu = plan_of(u, Gu, vertical=explicit, top_flux=-0.1, mode="write")
    a = pu._call[1]
    assert a[3:5] == (2, 1) and a[7] == 1e-2 and a[11:15] == (None,) * 4 and a[9] is not None and a[10] is None
    assert pu.top_flux[0].shape == (u.Ny + 2 * u.Hy, u.Nx + 2 * u.Hx) and float(pu.top_flux[0][0, 0]) == -0.1
    # "from_fields": a field's own FluxBoundaryCondition on its top or bottom side; any other class contributes nothing
    plane = torch.zeros((c.Ny + 2 * c.Hy, c.Nx + 2 * c.Hx), dtype=torch.float64)
    bcs = osg.FieldBoundaryConditions(top=osg.FluxBoundaryCondition(plane), bottom=osg.ValueBoundaryCondition(1.0))
    b = osg.CenterField(grid, boundary_conditions=bcs)
    pb = plan_of([c, b], [G, H_])
    assert pb.terms == 0 and pb.bottom_flux is None and pb.top_flux[0] is None and pb.top_flux[1] is plane and pb._call[1][10] is None
    assert plan_of([c, b], [G, H_], top_flux=[0.5, None], vertical=1.0).top_flux[1] is None                          # a list overrides the fields' own
    with pytest.raises(TypeError, match="nothing to compute"):
        plan_of([c, b], [G, H_], top_flux=None)
    reduced = osg.Field((osg.Center, osg.Center, None), grid)
    assert plan_of(c, G, bottom_flux=reduced).bottom_flux[0].data_ptr() == reduced.data.data_ptr()
    many = [osg.CenterField(grid) for _ in range(35)]
    outs = [osg.CenterField(grid) for _ in range(35)]
    m = plan_of(many, outs, horizontal=1.0, top_flux=[0.25] + [None] * 34)
    assert [x._call[1][2] for x in m._before] + [m._call[1][2]] == [16, 16, 3]
    assert all(x._call[1][9] is not None for x in (*m._before, m))                # every batch keeps its table: the group is the plan's
    out = D.DiffusiveTendencyPlan(c, G, vertical=torch.ones(4, dtype=torch.float64))
    assert out._call[1][8] == 1 and out._call[1][6] == out.vertical.data_ptr()


def test_the_table_of_the_libraries_is_as_the_parent_left_it(osg):
    """the library is staged BESIDE the table: fifteen entries, none of them this one, and csrc/Makefile does what the parent's does"""
    assert len(osg._lib.LIBRARIES) == 15 and "diffusion" not in osg._lib.LIBRARIES and not hasattr(osg._lib, "DIFFUSION_SIGNATURES")
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC], capture_output=True, text=True, check=True).stdout
    assert "diffusion" not in out.replace("vertical_diffusion", "") and "staged" not in out
    pinned = subprocess.run(["make", "-n", "-B", "-C", CSRC, "HIPCC=hipcc", "ARCH=gfx950"], capture_output=True, text=True, check=True).stdout
    printed = [line for line in pinned.splitlines() if not line.startswith("make")]
    parent = open(PARENT_MAKE).read().splitlines()
    changed = [line for line in difflib.unified_diff(parent, printed, "the parent's", "this tree's", lineterm="", n=0)]
    assert not changed, "make -n -B -C csrc no longer prints what the parent of the staged library printed:\n" + "\n".join(changed)
    lines = [line for line in subprocess.run(["make", "-n", "-B", "-C", STAGED, "DIFFUSION_TAG=_t", "DIFFUSION_FLAGS=-DTPG_X=1"], capture_output=True, text=True,
                                             check=True).stdout.splitlines() if not line.startswith("make")]
    compiles = [line for line in lines if "-c tpg_diffusion.hip" in line]
    assert len(compiles) == 1 and compiles[0].endswith("-c tpg_diffusion.hip -o tpg_diffusion_t.o")
    assert " -DTPG_X=1 " in compiles[0] and " -ffp-contract=off " in compiles[0] and " --offload-arch=gfx950 " in compiles[0] and " -I .. " in compiles[0]
    links = [line for line in lines if "-shared" in line]
    assert len(links) == 1 and " -Wl,--version-script=diffusion.map " in links[0]
    assert links[0].endswith("-o ../../libtripolar_hip_diffusion_t.so.tmp ../tpg_api.o tpg_diffusion_t.o")
    assert lines[-1] == "mv -f ../../libtripolar_hip_diffusion_t.so.tmp ../../libtripolar_hip_diffusion_t.so"
    body = open(os.path.join(STAGED, "tpg_diffusion.hip")).read()
    assert '#include "tpg_operator.hpp"' in body and "chunk_plan<T>" in body and "getenv" not in body
    assert body.count("__global__") == 1 and "__syncthreads" not in body and "atomic" not in body.replace("No atomics", "") and "hipMalloc" not in body
    import inspect
    import __graft_entry__
    source = inspect.getsource(__graft_entry__.build)
    assert 'os.path.join(csrc, "staged")' in source and "diffusion.diffusion_lib()" in source


def test_the_records_of_the_build():
    """nothing differs in an existing object; nothing of the new kernels in private memory, no LDS, no register spill"""
    import json
    diff = json.load(open(os.path.join(ROOT, "profiles", "diffusion", "isa_diff.json")))
    assert "tpg_vertical_diffusion.o" in diff and "tpg_advection.o" in diff and "tpg_grid.o" in diff and len(diff) >= 27
    for name, r in diff.items():
        assert r.get("code_object_identical", True), name
        assert not any(r.get(k) for k in ("differing", "metadata_differing", "only_old", "only_new", "renamed")), name
    res = json.load(open(os.path.join(ROOT, "profiles", "diffusion", "resources.json")))["kernels"]
    assert len(res) == 25 and all("k_diffusive_tendency" in k for k in res)       # 5 chunk forms x (3 groups without the horizontal group + 2 with it)
    for k, r in res.items():
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"], r["group_segment_fixed_size"],
                r["uses_dynamic_stack"]) == ("0", "0", "0", "0", "false"), k
        assert int(r["vgpr_count"]) + int(r["agpr_count"]) <= 256 and int(r["max_flat_workgroup_size"]) == 256, k
    tool = open(os.path.join(ROOT, "tools", "diffusion_argcheck.cpp")).read()
    assert "int main()" in tool and "-fsanitize=address,undefined" in tool and "tpg_diffusive_tendency(" in tool


def test_the_sanitizer_program_of_the_host_checks_builds_and_passes(tmp_path):
    """tools/diffusion_argcheck.cpp, a stand-alone host program with its own main, built as its header comment says with the address and
    undefined-behaviour sanitizers on the host side and run here, on the CPU: it exits 0 and prints its one line"""
    exe = str(tmp_path / "diffusion_argcheck")
    build = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                            "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tools", "diffusion_argcheck.cpp"), os.path.join(STAGED, "tpg_diffusion.hip"), os.path.join(CSRC, "tpg_api.hip"),
                            "-ldl", "-o", exe], capture_output=True, text=True, cwd=str(tmp_path))
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "diffusion_argcheck: every call refused in validation, with its status and message", run.stdout + run.stderr
