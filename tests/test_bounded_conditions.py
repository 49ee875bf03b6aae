"""No-flux south / bottom / top halos without a GPU: the Flux classification and its validation, the scope of fill_halo_regions,
how HaloFillPlan marshals tpg_fill_bounded_halos, the order-independence claim the post-pass rests on (C oracle + numpy), and the
argument checks of the C entry point (which precede any device work)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from orthogonalsphericalshellgrids.jl_amd.boundary_conditions import AbstractBoundaryConditionClassification, Periodic
from bounded_ref import BOTTOM, SOUTH, TOP, bounded_sequence, post_pass_sequence, random_field

LOCS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def host_grid(osg, size=(16, 12, 4), halo=(4, 4, 4), arch=None):
    """a tripolar grid whose (unused) arrays live in host memory: enough for Field construction and HaloFillPlan marshalling"""
    from orthogonalsphericalshellgrids.jl_amd.grids import (Bounded, OrthogonalSphericalShellGrid, PeriodicTopology, RightConnected,
                                                             Tripolar)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    z = torch.zeros(1, dtype=torch.float64)
    return OrthogonalSphericalShellGrid(architecture=arch or osg.GPU(), Nx=Nx, Ny=Ny, Nz=Nz, Hx=Hx, Hy=Hy, Hz=Hz, Lz=1.0,
                                        arrays={"lambda_cc": z}, z_faces=z, z_centers=z, radius=1.0,
                                        conformal_mapping=Tripolar(55, 70, -80), topology=(PeriodicTopology, RightConnected, Bounded))


def no_flux(osg, south=True, bottom=True, top=True):
    nf, per = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition
    return osg.FieldBoundaryConditions(west=per(), east=per(), south=nf() if south else None,
                                       bottom=nf() if bottom else None, top=nf() if top else None)


def test_flux_classification_and_constructors(osg):
    bc = osg.NoFluxBoundaryCondition()
    assert isinstance(bc.classification, osg.Flux) and bc.condition is None
    assert bc == osg.FluxBoundaryCondition(None) == osg.FluxBoundaryCondition()
    assert osg.FluxBoundaryCondition(2.5).condition == 2.5
    assert osg.bc_str(bc) == "Flux"


@pytest.mark.parametrize("loc,side", [
    (("Center", "Face", "Center"), "south"),      # v
    (("Face", "Face", "Center"), "south"),        # zeta
    (("Center", "Center", "Face"), "bottom"),     # ZFaceField
    (("Center", "Center", "Face"), "top"),
    (("Face", "Center", "Center"), "west"),       # u: Face in x
])
def test_flux_on_a_face_axis_is_refused_at_construction(osg, loc, side):
    grid = host_grid(osg)
    loc = tuple(getattr(osg, L) for L in loc)
    bcs = osg.FieldBoundaryConditions(**{side: osg.NoFluxBoundaryCondition()})
    with pytest.raises(ValueError, match="Cannot specify"):
        osg.Field(loc, grid, boundary_conditions=bcs)
    with pytest.raises(ValueError):
        osg.validate_boundary_condition_location(osg.FluxBoundaryCondition(1.0), osg.Face, side)
    assert osg.validate_boundary_condition_location(osg.NoFluxBoundaryCondition(), osg.Center, side) is None


@pytest.mark.parametrize("side", ["west", "east"])
def test_flux_in_x_is_still_refused(osg, side):
    grid = host_grid(osg)
    per = osg.PeriodicBoundaryCondition
    sides = {"west": per(), "east": per(), side: osg.NoFluxBoundaryCondition()}
    c = osg.CenterField(grid, boundary_conditions=osg.FieldBoundaryConditions(**sides))
    with pytest.raises(NotImplementedError, match="Periodic in x"):
        osg.halo_fill_plan([c])


class Value(AbstractBoundaryConditionClassification):
    """stand-in for Oceananigans' Value / Gradient / Open classifications, which stay Oceananigans' to fill"""


@pytest.mark.parametrize("side", ["south", "bottom", "top"])
@pytest.mark.parametrize("kind", ["unknown", "value", "periodic"])
def test_other_classifications_on_bounded_sides_are_still_refused(osg, side, kind):
    grid = host_grid(osg)
    per = osg.PeriodicBoundaryCondition
    bc = {"unknown": osg.BoundaryCondition(object(), 0.0), "value": osg.BoundaryCondition(Value(), 1.0), "periodic": per()}[kind]
    c = osg.CenterField(grid, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **{side: bc}))
    with pytest.raises(NotImplementedError):
        osg.halo_fill_plan([c])


def test_defaults_are_unchanged(osg):
    grid = host_grid(osg)
    for ctor in (osg.CenterField, osg.XFaceField, osg.YFaceField, osg.ZFaceField):
        b = ctor(grid).boundary_conditions
        assert b.south is None and b.bottom is None and b.top is None
        assert isinstance(b.west.classification, Periodic) and isinstance(b.east.classification, Periodic)
    plan = osg.halo_fill_plan([osg.CenterField(grid), osg.XFaceField(grid)])
    (_, calls, pending), = plan._steps
    assert [fn.__name__ for fn, *_ in calls] == ["tpg_fill_halo_regions"] and pending is None


def _fields(osg, grid):
    """the model's default fields: c, u south + bottom + top; v, zeta bottom + top (Face in y: no south condition)"""
    return [osg.CenterField(grid, boundary_conditions=no_flux(osg)), osg.XFaceField(grid, boundary_conditions=no_flux(osg)),
            osg.YFaceField(grid, boundary_conditions=no_flux(osg, south=False)),
            osg.Field((osg.Face, osg.Face, osg.Center), grid, boundary_conditions=no_flux(osg, south=False))]


def test_serial_plan_appends_one_bounded_call_after_the_horizontal_fill(osg):
    grid = host_grid(osg)
    fs = _fields(osg, grid)
    plan = osg.halo_fill_plan(fs)
    (_, calls, pending), = plan._steps
    assert pending is None and plan._post == [[]]
    assert [fn.__name__ for fn, *_ in calls] == ["tpg_fill_halo_regions", "tpg_fill_bounded_halos"]
    ptrs, n, sides, *rest = calls[1][1]
    assert n == 4 and list(sides) == [SOUTH | BOTTOM | TOP] * 2 + [BOTTOM | TOP] * 2
    assert [ptrs[k] for k in range(n)] == [f.data.data_ptr() for f in fs]
    assert tuple(rest) == (16, 12, 4, 4, 4, 4, osg._lib.TPG_F64)
    # a group without a zipper field takes the periodic pass alone, then the mirror
    c = osg.CenterField(grid, boundary_conditions=no_flux(osg, south=False, top=False))
    c.boundary_conditions.north = None
    (_, calls, _), = osg.halo_fill_plan([c])._steps
    assert [fn.__name__ for fn, *_ in calls] == ["tpg_periodic_x_fill", "tpg_fill_bounded_halos"]
    assert list(calls[1][1][2]) == [BOTTOM]


def test_band_plan_runs_the_mirror_after_the_seam_exchange(osg):
    """host-driven band branch: the mirror is a finish() call; only rank 0 keeps a physical (no-flux) south side"""
    R = 3
    for r in range(R):
        arch = osg.Distributed(osg.GPU(), osg.Partition(y=R), local_rank=r)
        grid = host_grid(osg, size=(16, 8, 4), arch=arch)
        fs = _fields(osg, grid)
        assert osg.is_flux(fs[0].boundary_conditions.south) == (r == 0)
        plan = osg.halo_fill_plan(fs, exchange=lambda *a: None)
        (_, calls, pending), = plan._steps
        assert pending is not None and "tpg_fill_bounded_halos" not in [fn.__name__ for fn, *_ in calls]
        (post,) = plan._post
        assert [fn.__name__ for fn, *_ in post] == ["tpg_fill_bounded_halos"]
        south = SOUTH if r == 0 else 0
        assert list(post[0][1][2]) == [south | BOTTOM | TOP] * 2 + [BOTTOM | TOP] * 2


@pytest.mark.parametrize("halo,size", [((4, 4, 4), (24, 12, 5)), ((5, 5, 5), (26, 14, 6)), ((3, 2, 1), (20, 10, 2))],
                         ids=["halo444", "halo555", "halo321"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_post_pass_order_gives_the_same_bits(oracle, halo, size, dtype):
    """zipper -> south (interior columns) -> bottom/top -> periodic x  ==  whole horizontal fill -> south (whole rows) -> bottom/top,
    bit for bit, for every location, sign and side combination: every pass is a signed copy along its own axis"""
    rng = np.random.default_rng(hash((halo, size, np.dtype(dtype).str)) % 2**32)
    for (xl, yl), sg, sides in itertools.product(LOCS, (1, -1), range(1, 8)):
        a = random_field(rng, size, halo, dtype)
        b, plain = a.copy(), a.copy()
        bounded_sequence(oracle, a, xl, yl, sg, size, halo, sides)
        post_pass_sequence(oracle, b, xl, yl, sg, size, halo, sides)
        assert np.array_equal(a, b), (xl, yl, sg, sides)
        assert not np.array_equal(a, oracle.fill_halo_regions(plain, xl, yl, sg, size, halo))     # the mirror wrote something


def test_argument_checks_precede_any_launch(osg):
    """bad side bits, a null table or a pointer off its element alignment: TPG_ERR_INVALID_ARGUMENT; a south mirror whose sources are
    not interior rows clear of the zipper (Ny <= Hy) or a bottom / top mirror with Nz < Hz: TPG_ERR_UNSUPPORTED.  The pointers are
    never dereferenced."""
    lib = osg._lib.lib()
    F64, F32 = osg._lib.TPG_F64, osg._lib.TPG_F32
    ptrs = (C.c_void_p * 2)(1 << 20, 2 << 20)
    sides = lambda *v: (C.c_uint8 * len(v))(*v)
    call = lambda s, geom, ft=F64, p=ptrs: lib.tpg_fill_bounded_halos(p, 2, s, *geom, ft, None)
    ok_geom = (16, 12, 4, 4, 4, 4)
    assert call(sides(8, 0), ok_geom) == -1
    assert call(sides(1, 0x81), ok_geom) == -1
    assert b"bits other than" in lib.tpg_last_error()
    assert call(None, ok_geom) == -1
    assert call(sides(1, 1), ok_geom, p=(C.c_void_p * 2)(1 << 20, (2 << 20) + 4)) == -1     # 4-B aligned Float64 field
    assert call(sides(1, 0), (16, 4, 4, 4, 4, 4)) == -5                                     # Ny == Hy with south
    assert b"Ny > Hy" in lib.tpg_last_error()
    assert call(sides(0, 2), (16, 12, 3, 4, 4, 4)) == -5                                    # Nz < Hz with bottom
    assert call(sides(4, 0), (16, 12, 3, 4, 4, 4), F32) == -5                               # ... or top
    assert b"Nz >= Hz" in lib.tpg_last_error()
    assert call(sides(0, 0), (16, 4, 3, 4, 4, 4)) == 0                                      # no side: nothing to check, nothing launched
    assert call(sides(2, 4), (16, 12, 1, 4, 4, 0)) == 0                                     # no z halo (reduced / windowed in z): a no-op
    assert call(sides(1, 1), (15, 12, 4, 4, 4, 4)) == -2                                    # the geometry checks of every fill
    assert lib.tpg_fill_bounded_halos(ptrs, 0, sides(1), *ok_geom, F64, None) == -1
