"""Open (impenetrable) south / bottom / top sides without a GPU: the classification and its constructors, which (location, side) pairs a
plan accepts and refuses, how HaloFillPlan marshals tpg_fill_open_faces FIRST on every path, the order identity of the pre-pass (C oracle +
numpy) and the argument checks of the C entry point (which precede any device work)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from bounded_ref import random_field
from open_ref import OPEN, library_sequence_open, oceananigans_sequence_open, open_faces
from test_value_gradient_conditions import bcs, names, vg_grid
from value_gradient_ref import GRADIENT, VALUE, periodic_rows

SOUTH, BOTTOM, TOP = 1, 2, 4
SENTINEL = 12345.0


def test_classification_constructors_and_equality(osg):
    o, imp = osg.OpenBoundaryCondition(0.25), osg.ImpenetrableBoundaryCondition()
    assert isinstance(o.classification, osg.Open) and o.condition == 0.25 and osg.is_open(o)
    assert isinstance(imp.classification, osg.Open) and imp.condition is None and osg.is_open(imp)
    assert imp == osg.OpenBoundaryCondition(None) == osg.OpenBoundaryCondition() == osg.BoundaryCondition(osg.Open(), None)
    assert o == osg.OpenBoundaryCondition(0.25) and o != osg.OpenBoundaryCondition(0.5) and o != osg.ValueBoundaryCondition(0.25)
    assert osg.Open() == osg.Open() and osg.Open() != osg.Flux() and osg.Flux() != osg.Open() and osg.Open() != osg.Value()
    assert hash(osg.Open()) == hash(osg.Open()) and repr(osg.Open()) == "Open()"
    assert osg.bc_str(o) == "Open" and osg.bc_str(imp) == "Open"
    assert not osg.is_flux(imp) and not osg.is_value(imp) and not osg.is_gradient(imp) and not osg.is_zipper(imp)
    assert not osg.is_open(osg.NoFluxBoundaryCondition()) and not osg.is_open(None) and not osg.is_open(osg.Open())
    # Open is valid at a Face on the side's axis (the boundary value is the field's own face value) -- and nowhere is it a Zipper
    for side in ("south", "bottom", "top"):
        assert osg.validate_boundary_condition_location(imp, osg.Face, side) is None


LOC = {"u": ("Face", "Center", "Center"), "v": ("Center", "Face", "Center"), "w": ("Center", "Center", "Face"),
       "c": ("Center", "Center", "Center"), "zeta": ("Face", "Face", "Center"), "eta": ("Center", "Center", None)}


def _loc(osg, name):
    return tuple(None if L is None else getattr(osg, L) for L in LOC[name])


def test_accepted_location_side_pairs(osg):
    grid = vg_grid(osg)
    imp = osg.ImpenetrableBoundaryCondition
    for name, sides in (("v", dict(south=imp())), ("w", dict(bottom=imp())), ("w", dict(top=imp())), ("w", dict(bottom=imp(), top=imp())),
                        ("w", dict(bottom=osg.OpenBoundaryCondition(0.5), top=imp(), south=osg.NoFluxBoundaryCondition()))):
        f = osg.Field(_loc(osg, name), grid, boundary_conditions=bcs(osg, **sides))
        (_, calls, _), = osg.halo_fill_plan([f])._steps
        assert names(calls)[0] == "tpg_fill_open_faces", (name, sides)


@pytest.mark.parametrize("name,side", [(n, s) for n in LOC for s in ("west", "east", "south", "north", "bottom", "top")
                                       if (n, s) not in (("v", "south"), ("w", "bottom"), ("w", "top"))])
def test_open_anywhere_else_is_refused_with_side_and_location(osg, name, side):
    grid = vg_grid(osg)
    per = osg.PeriodicBoundaryCondition
    sides = {"west": per(), "east": per(), side: osg.ImpenetrableBoundaryCondition()}
    f = osg.Field(_loc(osg, name), grid, boundary_conditions=osg.FieldBoundaryConditions(**sides))
    if side == "north":                                    # the Field constructor replaces a non-Zipper north side (serial grid)
        assert osg.is_zipper(f.boundary_conditions.north)
        osg.halo_fill_plan([f])
        return
    at = "(" + ", ".join("Nothing" if L is None else L for L in LOC[name]) + ")"
    with pytest.raises(NotImplementedError) as e:
        osg.halo_fill_plan([f])
    assert f"{side} boundary condition Open()" in str(e.value) and at in str(e.value)


def test_open_on_a_z_windowed_field_is_refused(osg):
    grid = vg_grid(osg)
    w = osg.ZFaceField(grid, indices=(slice(None), slice(None), range(1, 3)), boundary_conditions=bcs(osg, bottom=osg.ImpenetrableBoundaryCondition()))
    with pytest.raises(NotImplementedError, match=r"bottom boundary condition Open\(\) on a z-windowed field at \(Center, Center, Face\)"):
        osg.halo_fill_plan([w])
    v = osg.YFaceField(grid, indices=(slice(None), slice(None), 2), boundary_conditions=bcs(osg, south=osg.ImpenetrableBoundaryCondition()))
    with pytest.raises(NotImplementedError, match="south boundary condition .* z-windowed"):
        osg.halo_fill_plan([v])


@pytest.mark.parametrize("name,side", [("v", "south"), ("w", "bottom"), ("w", "top")])
def test_bad_conditions_are_refused_at_plan_build_with_the_expected_shape(osg, name, side):
    grid = vg_grid(osg)                                   # 16 x 12 x 4, halo 4: v south (4, 24); w bottom / top (20, 24)
    shape = (4, 24) if side == "south" else (20, 24)
    at = "(" + ", ".join(LOC[name]) + ")"
    f = osg.Field(_loc(osg, name), grid, boundary_conditions=bcs(osg, **{side: osg.OpenBoundaryCondition(lambda x, y, t: 0.0)}))
    with pytest.raises(NotImplementedError, match=r"\(%d, %d\)" % shape) as e:
        osg.halo_fill_plan([f])
    assert f"{side} boundary condition Open()" in str(e.value) and at in str(e.value) and "function-valued" in str(e.value)
    bad = [True, "1.0", torch.zeros(12, 16, dtype=torch.float64), torch.zeros(shape[1], dtype=torch.float64),
           torch.zeros(shape, dtype=torch.float32), torch.zeros(shape, dtype=torch.float64, device="meta"),
           torch.zeros(shape[::-1], dtype=torch.float64).t(), torch.zeros((5, 24) if side == "south" else (12, 24), dtype=torch.float64)]
    for cond in bad:
        f = osg.Field(_loc(osg, name), grid, boundary_conditions=bcs(osg, **{side: osg.OpenBoundaryCondition(cond)}))
        with pytest.raises(ValueError, match=r"\(%d, %d\)" % shape):
            osg.halo_fill_plan([f])
    for cond in (None, 0.5, 3, torch.tensor(0.5), torch.zeros(shape, dtype=torch.float64)):
        osg.halo_fill_plan([osg.Field(_loc(osg, name), grid, boundary_conditions=bcs(osg, **{side: osg.OpenBoundaryCondition(cond)}))])
    # a reduced field is a bottom / top condition only, and only at the field's own horizontal location on the same grid
    w0 = osg.Field((osg.Center, osg.Center, None), grid)
    f = osg.Field(_loc(osg, name), grid, boundary_conditions=bcs(osg, **{side: osg.OpenBoundaryCondition(w0)}))
    if side == "south":
        with pytest.raises(ValueError):
            osg.halo_fill_plan([f])
    else:
        (_, calls, _), = osg.halo_fill_plan([f])._steps
        assert calls[0][1][4][1 if side == "bottom" else 2] == w0.data.data_ptr()
        other = osg.Field((osg.Face, osg.Center, None), grid)
        with pytest.raises(ValueError):
            osg.halo_fill_plan([osg.Field(_loc(osg, name), grid, boundary_conditions=bcs(osg, **{side: osg.OpenBoundaryCondition(other)}))])


def _model_fields(osg, grid, v_south="default", w_bottom="default", w_top="default"):
    """u, v, w, T, S with a model's default sides: v south impenetrable, w bottom / top impenetrable, every Center side no-flux"""
    nf, imp = osg.NoFluxBoundaryCondition, osg.ImpenetrableBoundaryCondition
    pick = lambda x: imp() if isinstance(x, str) else x
    return [osg.XFaceField(grid, name="u", boundary_conditions=bcs(osg, nf(), nf(), nf())),
            osg.YFaceField(grid, name="v", boundary_conditions=bcs(osg, pick(v_south), nf(), nf())),
            osg.ZFaceField(grid, name="w", boundary_conditions=bcs(osg, nf(), pick(w_bottom), pick(w_top))),
            osg.CenterField(grid, name="T", boundary_conditions=bcs(osg, nf(), nf(), nf())),
            osg.CenterField(grid, name="S", boundary_conditions=bcs(osg, nf(), nf(), nf()))]


def test_serial_plan_puts_the_open_call_first(osg):
    grid = vg_grid(osg)
    imp = osg.ImpenetrableBoundaryCondition
    v = osg.YFaceField(grid, boundary_conditions=bcs(osg, south=imp()))
    (_, calls, pending), = osg.halo_fill_plan([v])._steps
    assert pending is None and names(calls) == ["tpg_fill_open_faces", "tpg_fill_halo_regions"]
    ptrs, n, sides, values, conds, *rest = calls[0][1]
    assert n == 1 and ptrs[0] == v.data.data_ptr() and list(sides) == [SOUTH] and list(values) == [0.0] * 3 and list(conds) == [None] * 3
    assert tuple(rest) == (16, 12, 4, 4, 4, 4, osg._lib.TPG_F64)
    w = osg.ZFaceField(grid, boundary_conditions=bcs(osg, bottom=imp(), top=osg.OpenBoundaryCondition(0.1)))
    (_, calls, _), = osg.halo_fill_plan([w])._steps
    assert names(calls) == ["tpg_fill_open_faces", "tpg_fill_halo_regions"]
    ptrs, n, sides, values, conds, *rest = calls[0][1]
    assert list(sides) == [BOTTOM | TOP] and list(values) == [0.0, 0.0, 0.1] and tuple(rest) == (16, 12, 5, 4, 4, 4, osg._lib.TPG_F64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_default_model_tuple_is_two_groups_with_open_first(osg, dtype):
    """(u, v, w, T, S): the four Nz-level fields are one geometry group, w (Nz + 1 levels) another; each group's Open call is its first,
    and the tables carry scalars rounded once to the field type and the condition tensors' pointers"""
    grid = vg_grid(osg, dtype=dtype)
    vs = torch.zeros(4, 24, dtype=dtype)
    wt = torch.zeros(20, 24, dtype=dtype)
    fs = _model_fields(osg, grid, v_south=osg.OpenBoundaryCondition(vs), w_bottom=osg.OpenBoundaryCondition(0.1),
                       w_top=osg.OpenBoundaryCondition(wt))
    u, v, w, T, S = fs
    plan = osg.halo_fill_plan(fs)
    (_, c4, p4), (_, cw, pw) = plan._steps
    assert p4 is None and pw is None and plan._post == [[], []]
    assert names(c4) == ["tpg_fill_open_faces", "tpg_fill_halo_regions", "tpg_fill_bounded_halos"]
    assert names(cw) == ["tpg_fill_open_faces", "tpg_fill_halo_regions", "tpg_fill_bounded_halos"]
    ptrs, n, sides, values, conds, *rest = c4[0][1]
    assert n == 4 and [ptrs[k] for k in range(4)] == [f.data.data_ptr() for f in (u, v, T, S)]
    assert list(sides) == [0, SOUTH, 0, 0] and list(values) == [0.0] * 12
    assert list(conds) == [None] * 3 + [vs.data_ptr(), None, None] + [None] * 6
    assert tuple(rest) == (16, 12, 4, 4, 4, 4, osg._lib.ft_of(dtype))
    assert list(c4[2][1][2]) == [7, 6, 7, 7]                                  # the no-flux mirror of the same group is what it was
    ptrs, n, sides, values, conds, *rest = cw[0][1]
    npt = np.float32 if dtype == torch.float32 else np.float64
    assert n == 1 and ptrs[0] == w.data.data_ptr() and list(sides) == [BOTTOM | TOP]
    assert list(values) == [0.0, float(npt(0.1)), 0.0] and list(conds) == [None, None, wt.data_ptr()]
    assert tuple(rest) == (16, 12, 5, 4, 4, 4, osg._lib.ft_of(dtype)) and list(cw[2][1][2]) == [SOUTH]
    assert any(t is vs for t in plan._held) and any(t is wt for t in plan._held)
    assert not plan.is_distributed


def test_with_value_gradient_sides_the_open_call_still_leads(osg):
    grid = vg_grid(osg)
    V, G, nf, imp = osg.ValueBoundaryCondition, osg.GradientBoundaryCondition, osg.NoFluxBoundaryCondition, osg.ImpenetrableBoundaryCondition
    fs = [osg.YFaceField(grid, boundary_conditions=bcs(osg, south=imp(), bottom=G(1e-3), top=V(2.0))),
          osg.CenterField(grid, boundary_conditions=bcs(osg, south=V(1.0), bottom=nf(), top=nf()))]
    (_, calls, _), = osg.halo_fill_plan(fs)._steps
    assert names(calls) == ["tpg_fill_open_faces", "tpg_fill_halo_regions", "tpg_fill_value_gradient_halos", "tpg_fill_bounded_halos",
                            "tpg_fill_value_gradient_halos"]


def test_plans_without_open_sides_issue_what_they_issued(osg):
    grid = vg_grid(osg)
    nf = osg.NoFluxBoundaryCondition
    fs = _model_fields(osg, grid, v_south=None, w_bottom=None, w_top=None)
    plan = osg.halo_fill_plan(fs)
    for _, calls, _ in plan._steps:
        assert names(calls) == ["tpg_fill_halo_regions", "tpg_fill_bounded_halos"]
    (_, calls, _), = osg.halo_fill_plan([osg.CenterField(grid)])._steps
    assert names(calls) == ["tpg_fill_halo_regions"]
    (_, calls, _), = osg.halo_fill_plan([osg.CenterField(grid, boundary_conditions=bcs(osg, nf(), osg.ValueBoundaryCondition(1.0), nf()))])._steps
    assert names(calls) == ["tpg_fill_halo_regions", "tpg_fill_bounded_halos", "tpg_fill_value_gradient_halos"]


def test_band_plans_issue_the_open_call_before_the_local_fill_never_in_finish(osg):
    """host-driven band branch: the south wall is rank 0's only; bottom / top are every rank's, on its own rows"""
    R = 3
    for r in range(R):
        arch = osg.Distributed(osg.GPU(), osg.Partition(y=R), local_rank=r)
        grid = vg_grid(osg, size=(16, 8, 4), arch=arch)
        wt = torch.zeros(8 + 8, 24, dtype=torch.float64)
        fs = _model_fields(osg, grid, w_top=osg.OpenBoundaryCondition(wt))
        u, v, w, T, S = fs
        assert osg.is_open(v.boundary_conditions.south) == (r == 0)
        plan = osg.halo_fill_plan(fs, exchange=lambda *a: None)
        (_, c4, p4), (_, cw, pw) = plan._steps
        post4, postw = plan._post
        assert p4 is not None and pw is not None
        zipper = ["tpg_fill_halo_regions"] if r == R - 1 else ["tpg_periodic_x_fill"]
        assert names(c4) == (["tpg_fill_open_faces"] if r == 0 else []) + zipper, r
        assert names(cw) == ["tpg_fill_open_faces"] + zipper, r
        assert names(post4) == ["tpg_fill_bounded_halos"] and "tpg_fill_open_faces" not in names(post4) + names(postw)
        assert names(postw) == (["tpg_fill_bounded_halos"] if r == 0 else [])
        if r == 0:
            assert list(c4[0][1][2]) == [0, SOUTH, 0, 0]
        assert list(cw[0][1][2]) == [BOTTOM | TOP] and cw[0][1][4][2] == wt.data_ptr()
        assert plan.is_distributed


@pytest.mark.parametrize("pack_free", [False, True])
def test_rccl_path_issues_the_open_call_before_the_one_call_fill(osg, pack_free):
    """the production branch's marshalling with a stub communicator (the pipelined form needs a device stream: tests/test_gpu_open_fill.py)"""
    from orthogonalsphericalshellgrids.jl_amd.distributed import RcclComm
    R = 3
    for r in range(R):
        arch = osg.Distributed(osg.GPU(), osg.Partition(y=R), local_rank=r, rccl_comm=RcclComm(C.c_void_p(0xC0FFEE), r, R))
        grid = vg_grid(osg, size=(16, 8, 4), arch=arch)
        fs = _model_fields(osg, grid)
        plan = osg.halo_fill_plan(fs, pack_free=pack_free)
        one_call = "tpg_fill_halo_regions_distributed"
        (_, c4, p4), (_, cw, pw) = plan._steps
        assert p4 is None and pw is None and plan._post == [[], []]
        assert names(c4) == (["tpg_fill_open_faces"] if r == 0 else []) + [one_call, "tpg_fill_bounded_halos"], r
        assert names(cw) == ["tpg_fill_open_faces", one_call] + (["tpg_fill_bounded_halos"] if r == 0 else []), r


# ---- the order identity -----------------------------------------------------------------------------------------------------------
def _spec(kind, rng, rows, size, halo, dtype, tensor):
    if kind is None or kind == "flux":
        return kind
    k = {"value": VALUE, "gradient": GRADIENT, "open": OPEN}[kind]
    return (k, periodic_rows(rng, rows, size, halo, dtype) if tensor else np.asarray(rng.uniform(-1, 1), dtype=dtype))


def _sentinel_halos(a, size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    keep = a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx].copy()
    a[...] = SENTINEL
    a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = keep
    return a


@pytest.mark.parametrize("halo,size", [((4, 4, 4), (24, 12, 5)), ((5, 5, 5), (26, 14, 6)), ((3, 2, 1), (20, 10, 2))],
                         ids=["halo444", "halo555", "halo321"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pre_pass_order_gives_the_same_bits(oracle, halo, size, dtype):
    """open write (interior columns) -> zipper -> south -> bottom / top -> periodic x  ==  open write (whole rows) -> whole horizontal
    fill -> VG south -> no-flux mirror -> VG bottom / top, bit for bit on the whole parent: v (south Open; every {none, Flux, Value,
    Gradient} on bottom and top) and w (bottom and / or top Open on Nz + 1 levels; every such class on south and on the z side Open
    leaves free), signs +1 / -1, scalar and x-periodic array conditions, every halo cell a sentinel beforehand"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(hash((halo, size, np.dtype(dtype).str)) % 2**32)
    dy_row = periodic_rows(rng, 1, size, halo, dtype)[0] * dtype(5e4)
    dz = (dtype(0.37), dtype(1.9))
    other = [None, "flux", "value", "gradient"]
    cases = [((0, 1), size, ("open", kb, kt)) for kb in other for kt in other]                                   # v
    wsize = (Nx, Ny, Nz + 1)
    cases += [((0, 0), wsize, (ks, kb, kt)) for ks in other
              for kb, kt in [("open", "open")] + [("open", k) for k in other] + [(k, "open") for k in other]]       # w
    ran = 0
    for ((xl, yl), sz, (ks, kb, kt)), sg, tensor in itertools.product(cases, (1, -1), (False, True)):
        nz = sz[2]
        south = _spec(ks, rng, nz, sz, halo, dtype, tensor)
        bottom = _spec(kb, rng, Ny + 2 * Hy, sz, halo, dtype, tensor)
        top = _spec(kt, rng, Ny + 2 * Hy, sz, halo, dtype, tensor)
        a = _sentinel_halos(random_field(rng, sz, halo, dtype), sz, halo)
        b, plain = a.copy(), a.copy()
        oceananigans_sequence_open(oracle, a, xl, yl, sg, sz, halo, south, bottom, top, dy_row, dz)
        library_sequence_open(oracle, b, xl, yl, sg, sz, halo, south, bottom, top, dy_row, dz)
        assert np.array_equal(a, b), (xl, yl, sg, ks, kb, kt, tensor)
        # the face cells hold the condition, and the pass is not a no-op
        want = open_faces(plain.copy(), sz, halo, *(s[1] if isinstance(s, tuple) and s[0] == OPEN else None for s in (south, bottom, top)),
                          slice(Hx, Hx + Nx))
        inner = (slice(Hz, Hz + nz), slice(Hy, Hy + Ny - 1), slice(Hx, Hx + Nx))             # row Ny is the zipper's
        assert np.array_equal(b[inner], want[inner]) and not np.array_equal(want, plain)
        ran += 1
    assert ran == (16 + 4 * 9) * 2 * 2


def test_reference_writes_only_the_documented_cells():
    size, halo = (8, 6, 3), (2, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    a = np.full((Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), SENTINEL)
    cs = np.arange(Nz * 12, dtype=np.float64).reshape(Nz, 12)
    cz = np.arange(10 * 12, dtype=np.float64).reshape(10, 12) + 1000
    open_faces(a, size, halo, cs, cz, -cz)
    changed = a != SENTINEL
    assert changed[Hz:Hz + Nz, Hy].all() and changed[Hz, Hy:Hy + Ny].all() and changed[Hz + Nz - 1, Hy:Hy + Ny].all()
    assert changed.sum() == (Nz - 2) * 12 + 2 * Ny * 12
    assert np.array_equal(a[Hz + 1, Hy], cs[1]) and np.array_equal(a[Hz, Hy:Hy + Ny], cz[Hy:Hy + Ny])      # the z side owns the shared row
    assert np.array_equal(a[Hz + Nz - 1, Hy:Hy + Ny], -cz[Hy:Hy + Ny])


# ---- the C entry point's argument checks ---------------------------------------------------------------------------------------------
def test_argument_checks_precede_any_launch(osg):
    """every error is returned before a launch: the pointers are never dereferenced"""
    lib = osg._lib.lib()
    F64, F32 = osg._lib.TPG_F64, osg._lib.TPG_F32
    ptrs = (C.c_void_p * 2)(1 << 20, 2 << 20)
    sides = lambda *v: (C.c_uint8 * 2)(*v)
    vals = (C.c_double * 6)()
    conds = lambda *v: (C.c_void_p * 6)(*v)
    ok = (16, 12, 4, 4, 4, 4)

    def call(s, geom=ok, ft=F64, p=ptrs, c=None, v=vals, n=2):
        return lib.tpg_fill_open_faces(p, n, s, v, conds() if c is None else c, *geom, ft, None)

    for bad in (8, 16, SOUTH | 8, 255):
        assert call(sides(0, bad)) == -1, bad
        assert b"bits other than" in lib.tpg_last_error()
    assert call(None) == -1 and b"null sides, values or conditions table" in lib.tpg_last_error()
    assert call(sides(SOUTH), v=None) == -1 and b"null sides" in lib.tpg_last_error()
    assert lib.tpg_fill_open_faces(ptrs, 2, sides(SOUTH), vals, None, *ok, F64, None) == -1
    assert call(sides(0, TOP), p=(C.c_void_p * 2)(1 << 20, (2 << 20) + 4)) == -1                   # a Float64 field 4-B aligned
    assert b"field 1: pointer not aligned" in lib.tpg_last_error()
    assert call(sides(TOP), p=(C.c_void_p * 2)(1 << 20, (2 << 20) + 2), ft=F32) == -1              # ... even a field without a side
    assert call(sides(0, TOP), c=conds(0, 0, 0, 0, 0, (4 << 20) + 2), ft=F32) == -1                # a condition off its alignment
    assert b"field 1 side 2: condition pointer" in lib.tpg_last_error()
    assert call(sides(SOUTH), geom=(16, 1, 4, 4, 1, 4)) == -5 and b"Ny >= 2" in lib.tpg_last_error()
    assert call(sides(0, BOTTOM | TOP), geom=(16, 12, 1, 4, 4, 4)) == -5 and b"Nz >= 2" in lib.tpg_last_error()
    assert call(sides(SOUTH | BOTTOM | TOP), geom=(46340, 46000, 2000, 0, 0, 0)) == -5             # 94000 rows x 23170 chunks >= 2^31
    assert b"Open faces too large for 32-bit" in lib.tpg_last_error()
    assert call(sides(0, 0)) == 0                                                                   # no field with a side: no launch
    assert call(sides(0, 0), geom=(16, 1, 1, 4, 1, 4)) == 0
    assert call(sides(SOUTH), geom=(15, 12, 4, 4, 4, 4)) == -2                                      # the geometry checks of every fill
    assert call(sides(SOUTH), ft=7) == -1 and call(sides(SOUTH), n=0) == -1
    assert call(sides(SOUTH), p=(C.c_void_p * 2)(1 << 20, None)) == -1 and b"null field 1" in lib.tpg_last_error()
