"""Value / Gradient south / bottom / top halos without a GPU: the classifications, constructors and their validation, the conditions a plan
accepts and refuses, how HaloFillPlan marshals tpg_fill_value_gradient_halos around the no-flux mirror, the order-independence claim of the
post-passes (C oracle + numpy), the argument checks of the C entry point (which precede any device work), the z spacings, and the reference's
own physics."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from orthogonalsphericalshellgrids.jl_amd.boundary_conditions import AbstractBoundaryConditionClassification
from value_gradient_ref import GRADIENT, VALUE, oceananigans_sequence, periodic_rows, post_pass_sequence, south_vg, z_vg
from bounded_ref import random_field

LOCS = [(0, 0), (1, 0), (0, 1), (1, 1)]
SOUTH, BOTTOM, TOP = 1, 2, 4


def vg_grid(osg, size=(16, 12, 4), halo=(4, 4, 4), arch=None, dtype=torch.float64, z=(0, 1)):
    """a tripolar grid whose arrays live in host memory, with a dy_cf array: enough for Field construction and plan marshalling"""
    from orthogonalsphericalshellgrids.jl_amd.grids import (Bounded, OrthogonalSphericalShellGrid, PeriodicTopology, RightConnected,
                                                             Tripolar)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    zero = torch.zeros(1, dtype=dtype)
    dy = torch.arange((Ny + 2 * Hy) * (Nx + 2 * Hx), dtype=dtype).view(Ny + 2 * Hy, Nx + 2 * Hx) + 1
    return OrthogonalSphericalShellGrid(architecture=arch or osg.GPU(), Nx=Nx, Ny=Ny, Nz=Nz, Hx=Hx, Hy=Hy, Hz=Hz, Lz=1.0,
                                        arrays={"lambda_cc": zero, "dy_cf": dy}, z_faces=zero, z_centers=zero, radius=1.0,
                                        conformal_mapping=Tripolar(55, 70, -80), topology=(PeriodicTopology, RightConnected, Bounded),
                                        dtype=dtype, z_spec=z)


def bcs(osg, south=None, bottom=None, top=None):
    per = osg.PeriodicBoundaryCondition
    return osg.FieldBoundaryConditions(west=per(), east=per(), south=south, bottom=bottom, top=top)


def names(calls):
    return [fn.__name__ for fn, *_ in calls]


def test_constructors_and_equality(osg):
    v, g = osg.ValueBoundaryCondition(2.5), osg.GradientBoundaryCondition(-1e-3)
    assert isinstance(v.classification, osg.Value) and v.condition == 2.5 and osg.is_value(v) and not osg.is_gradient(v)
    assert isinstance(g.classification, osg.Gradient) and g.condition == -1e-3 and osg.is_gradient(g) and not osg.is_value(g)
    assert v == osg.ValueBoundaryCondition(2.5) and v != osg.ValueBoundaryCondition(2.0) and v != osg.GradientBoundaryCondition(2.5)
    assert osg.Value() == osg.Value() and osg.Gradient() == osg.Gradient() and osg.Value() != osg.Gradient()
    assert hash(osg.Value()) == hash(osg.Value())
    assert osg.bc_str(v) == "Value" and osg.bc_str(g) == "Gradient"
    assert not osg.is_flux(v) and not osg.is_value(osg.NoFluxBoundaryCondition())


@pytest.mark.parametrize("ctor", ["ValueBoundaryCondition", "GradientBoundaryCondition"])
@pytest.mark.parametrize("loc,side", [
    (("Center", "Face", "Center"), "south"),      # v
    (("Face", "Face", "Center"), "south"),        # zeta
    (("Center", "Center", "Face"), "bottom"),     # ZFaceField
    (("Center", "Center", "Face"), "top"),
])
def test_value_and_gradient_on_a_face_axis_are_refused_at_construction(osg, ctor, loc, side):
    grid = vg_grid(osg)
    loc = tuple(getattr(osg, L) for L in loc)
    bc = getattr(osg, ctor)(1.0)
    with pytest.raises(ValueError, match="Cannot specify"):
        osg.Field(loc, grid, boundary_conditions=osg.FieldBoundaryConditions(**{side: bc}))
    assert osg.validate_boundary_condition_location(bc, osg.Center, side) is None


@pytest.mark.parametrize("side", ["west", "east"])
def test_value_in_x_is_still_refused(osg, side):
    per = osg.PeriodicBoundaryCondition
    sides = {"west": per(), "east": per(), side: osg.ValueBoundaryCondition(1.0)}
    c = osg.CenterField(vg_grid(osg), boundary_conditions=osg.FieldBoundaryConditions(**sides))
    with pytest.raises(NotImplementedError, match="Periodic in x"):
        osg.halo_fill_plan([c])


class Open(AbstractBoundaryConditionClassification):
    """stand-in for Oceananigans' Open classification, which stays Oceananigans' to fill"""


class Value(AbstractBoundaryConditionClassification):
    """a foreign class that is only NAMED Value: not the library's classification"""


@pytest.mark.parametrize("side", ["south", "bottom", "top"])
@pytest.mark.parametrize("cls", [Open, Value])
def test_open_and_stand_in_classes_are_still_refused(osg, side, cls):
    c = osg.CenterField(vg_grid(osg), boundary_conditions=bcs(osg, **{side: osg.BoundaryCondition(cls(), 1.0)}))
    with pytest.raises(NotImplementedError):
        osg.halo_fill_plan([c])


@pytest.mark.parametrize("side", ["south", "bottom", "top"])
def test_bad_conditions_are_refused_at_plan_build_with_the_expected_shape(osg, side):
    grid = vg_grid(osg)                                   # 16 x 12 x 4, halo 4: south (4, 24), bottom / top (20, 24)
    shape = (4, 24) if side == "south" else (20, 24)
    bad = [lambda x, y, t: 0.0, None, True, "1.0", torch.zeros(12, 16, dtype=torch.float64), torch.zeros(shape[1], dtype=torch.float64),
           torch.zeros(shape, dtype=torch.float32), torch.zeros(shape, dtype=torch.float64, device="meta"),
           torch.zeros(shape[::-1], dtype=torch.float64).t()]
    for cond in bad:
        for ctor in (osg.ValueBoundaryCondition, osg.GradientBoundaryCondition):
            c = osg.CenterField(grid, boundary_conditions=bcs(osg, **{side: ctor(cond)}))
            with pytest.raises(ValueError, match=r"\(%d, %d\)" % shape):
                osg.halo_fill_plan([c])
    ok = osg.CenterField(grid, boundary_conditions=bcs(osg, **{side: osg.ValueBoundaryCondition(torch.zeros(shape, dtype=torch.float64))}))
    osg.halo_fill_plan([ok])


def test_reduced_field_conditions(osg):
    grid, other = vg_grid(osg), vg_grid(osg)
    T0 = osg.Field((osg.Center, osg.Center, None), grid)
    c = osg.CenterField(grid, boundary_conditions=bcs(osg, top=osg.ValueBoundaryCondition(T0), bottom=osg.GradientBoundaryCondition(T0)))
    (_, calls, _), = osg.halo_fill_plan([c])._steps
    assert names(calls) == ["tpg_fill_halo_regions", "tpg_fill_value_gradient_halos"]
    conds = calls[1][1][5]
    assert conds[1] == conds[2] == T0.data.data_ptr()
    for cond, side in [(osg.Field((osg.Face, osg.Center, None), grid), "top"), (osg.Field((osg.Center, osg.Center, None), other), "top"),
                       (T0, "south")]:
        f = osg.CenterField(grid, boundary_conditions=bcs(osg, **{side: osg.ValueBoundaryCondition(cond)}))
        with pytest.raises(ValueError):
            osg.halo_fill_plan([f])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scalar_conditions_are_rounded_once_to_the_field_type(osg, dtype):
    grid = vg_grid(osg, dtype=dtype)
    c = osg.CenterField(grid, boundary_conditions=bcs(osg, south=osg.ValueBoundaryCondition(0.1),
                                                      bottom=osg.GradientBoundaryCondition(torch.tensor(1 / 3, dtype=torch.float64)),
                                                      top=osg.ValueBoundaryCondition(7)))
    (_, calls, _), = osg.halo_fill_plan([c])._steps
    values = list(calls[1][1][4])
    npt = np.float32 if dtype == torch.float32 else np.float64
    assert values == [float(npt(0.1)), float(npt(1 / 3)), 7.0]
    if dtype == torch.float32:
        assert values[0] != 0.1
    assert list(calls[1][1][5]) == [None, None, None]


def test_serial_plan_order_south_then_mirror_then_z(osg):
    grid = vg_grid(osg)
    Tb = torch.zeros(20, 24, dtype=torch.float64)
    nf = osg.NoFluxBoundaryCondition
    fs = [osg.CenterField(grid, boundary_conditions=bcs(osg, south=osg.GradientBoundaryCondition(1e-3), bottom=nf(),
                                                        top=osg.ValueBoundaryCondition(Tb))),
          osg.XFaceField(grid, boundary_conditions=bcs(osg, south=nf(), bottom=osg.ValueBoundaryCondition(2.0), top=nf())),
          osg.YFaceField(grid, boundary_conditions=bcs(osg, bottom=nf(), top=nf()))]
    plan = osg.halo_fill_plan(fs)
    (_, calls, pending), = plan._steps
    assert pending is None and plan._post == [[]]
    assert names(calls) == ["tpg_fill_halo_regions", "tpg_fill_value_gradient_halos", "tpg_fill_bounded_halos",
                            "tpg_fill_value_gradient_halos"]
    ptrs, n, pss, kinds, values, conds, dy, dzb, dzt, *rest = calls[1][1]
    assert n == 3 and pss == SOUTH and [ptrs[k] for k in range(n)] == [f.data.data_ptr() for f in fs]
    assert list(kinds) == [GRADIENT, 0, VALUE, 0, VALUE, 0, 0, 0, 0]
    assert list(values)[:5] == [1e-3, 0.0, 0.0, 0.0, 2.0]
    assert conds[2] == Tb.data_ptr() and conds[0] is None
    assert dy.value == grid.arrays["dy_cf"].data_ptr()
    assert (dzb, dzt) == (0.25, 0.25) and tuple(rest) == (16, 12, 4, 4, 4, 4, osg._lib.TPG_F64)
    assert calls[3][1][2] == BOTTOM | TOP and calls[3][1][3:] == calls[1][1][3:]
    assert list(calls[2][1][2]) == [BOTTOM, SOUTH | TOP, BOTTOM | TOP]
    assert plan._held and any(t is Tb for t in plan._held)
    assert not plan.is_distributed


def test_only_the_needed_passes_appear(osg):
    grid = vg_grid(osg)
    cases = [({"top": osg.ValueBoundaryCondition(1.0)}, ["tpg_fill_halo_regions", "tpg_fill_value_gradient_halos"], TOP),
             ({"bottom": osg.GradientBoundaryCondition(1.0)}, ["tpg_fill_halo_regions", "tpg_fill_value_gradient_halos"], BOTTOM),
             ({"south": osg.ValueBoundaryCondition(1.0)}, ["tpg_fill_halo_regions", "tpg_fill_value_gradient_halos"], SOUTH),
             ({"south": osg.ValueBoundaryCondition(1.0), "top": osg.NoFluxBoundaryCondition()},
              ["tpg_fill_halo_regions", "tpg_fill_value_gradient_halos", "tpg_fill_bounded_halos"], SOUTH)]
    for sides, want, pss in cases:
        (_, calls, _), = osg.halo_fill_plan([osg.CenterField(grid, boundary_conditions=bcs(osg, **sides))])._steps
        assert names(calls) == want and calls[1][1][2] == pss
    # a Flux-only group issues exactly what it issued before Value / Gradient existed
    nf = osg.NoFluxBoundaryCondition
    (_, calls, _), = osg.halo_fill_plan([osg.CenterField(grid, boundary_conditions=bcs(osg, nf(), nf(), nf()))])._steps
    assert names(calls) == ["tpg_fill_halo_regions", "tpg_fill_bounded_halos"]
    # the z spacings are computed only for a group with a z side: a south-only group needs no z_spec
    g2 = vg_grid(osg, z=None)
    osg.halo_fill_plan([osg.CenterField(g2, boundary_conditions=bcs(osg, south=osg.ValueBoundaryCondition(1.0)))])
    with pytest.raises(TypeError):
        osg.halo_fill_plan([osg.CenterField(g2, boundary_conditions=bcs(osg, top=osg.ValueBoundaryCondition(1.0)))])


def test_band_plan_runs_both_passes_after_the_seam_exchange(osg):
    """host-driven band branch: south VG (rank 0 only), mirror, z VG are finish() calls; bottom / top tensors are band-local"""
    R = 3
    for r in range(R):
        arch = osg.Distributed(osg.GPU(), osg.Partition(y=R), local_rank=r)
        grid = vg_grid(osg, size=(16, 8, 4), arch=arch)
        Tt = torch.zeros(8 + 8, 24, dtype=torch.float64)
        c = osg.CenterField(grid, boundary_conditions=bcs(osg, south=osg.GradientBoundaryCondition(0.5),
                                                          bottom=osg.NoFluxBoundaryCondition(), top=osg.ValueBoundaryCondition(Tt)))
        assert osg.is_gradient(c.boundary_conditions.south) == (r == 0)
        plan = osg.halo_fill_plan([c], exchange=lambda *a: None)
        (_, calls, pending), = plan._steps
        assert pending is not None and "tpg_fill_value_gradient_halos" not in names(calls)
        (post,) = plan._post
        want = (["tpg_fill_value_gradient_halos"] if r == 0 else []) + ["tpg_fill_bounded_halos", "tpg_fill_value_gradient_halos"]
        assert names(post) == want
        assert post[-1][1][2] == TOP and post[-1][1][5][2] == Tt.data_ptr()


def _spec(kind, rng, rows, size, halo, dtype, tensor):
    """a side spec for the reference: ('flux'), (kind, scalar) or (kind, x-periodic array)"""
    if kind == "flux":
        return "flux"
    k = VALUE if kind == "value" else GRADIENT
    return (k, periodic_rows(rng, rows, size, halo, dtype) if tensor else np.asarray(rng.uniform(-1, 1), dtype=dtype))


@pytest.mark.parametrize("halo,size", [((4, 4, 4), (24, 12, 5)), ((5, 5, 5), (26, 14, 6)), ((3, 2, 1), (20, 10, 2))],
                         ids=["halo444", "halo555", "halo321"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_post_pass_order_gives_the_same_bits(oracle, halo, size, dtype):
    """zipper -> south (interior columns) -> bottom/top -> periodic x  ==  whole horizontal fill -> VG south (whole rows) -> no-flux
    mirror -> VG bottom / top, bit for bit, for every location, sign and {none, Flux, Value, Gradient} per side, with x-periodic
    condition arrays and dy_cf"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(hash((halo, size, np.dtype(dtype).str)) % 2**32)
    dy_row = periodic_rows(rng, 1, size, halo, dtype)[0] * dtype(5e4)
    dz = (dtype(0.37), dtype(1.9))
    kinds = [None, "flux", "value", "gradient"]
    written = 0
    for (xl, yl), sg, (ks, kb, kt), tensor in itertools.product(LOCS, (1, -1), itertools.product(kinds, repeat=3), (False, True)):
        if ks is None and kb is None and kt is None:
            continue
        south = None if ks is None else _spec(ks, rng, Nz, size, halo, dtype, tensor)
        bottom = None if kb is None else _spec(kb, rng, Ny + 2 * Hy, size, halo, dtype, tensor)
        top = None if kt is None else _spec(kt, rng, Ny + 2 * Hy, size, halo, dtype, tensor)
        a = random_field(rng, size, halo, dtype)
        b, plain = a.copy(), a.copy()
        oceananigans_sequence(oracle, a, xl, yl, sg, size, halo, south, bottom, top, dy_row, dz)
        post_pass_sequence(oracle, b, xl, yl, sg, size, halo, south, bottom, top, dy_row, dz)
        assert np.array_equal(a, b), (xl, yl, sg, ks, kb, kt, tensor)
        written += not np.array_equal(a, oracle.fill_halo_regions(plain, xl, yl, sg, size, halo))
    assert written == 4 * 2 * 63 * 2


def test_argument_checks_precede_any_launch(osg):
    """every error is returned before a launch: the pointers are never dereferenced"""
    lib = osg._lib.lib()
    F64, F32 = osg._lib.TPG_F64, osg._lib.TPG_F32
    ptrs = (C.c_void_p * 2)(1 << 20, 2 << 20)
    kinds = lambda *v: (C.c_uint8 * 6)(*v)
    vals = (C.c_double * 6)()
    conds = lambda *v: (C.c_void_p * 6)(*v)
    dy = C.c_void_p(3 << 20)
    ok = (16, 12, 4, 4, 4, 4)

    def call(pss, k, geom=ok, ft=F64, p=ptrs, c=None, d=dy, v=vals):
        return lib.tpg_fill_value_gradient_halos(p, 2, pss, k, v, conds() if c is None else c, d, 0.5, 0.5, *geom, ft, None)

    for pss in (0, 8, SOUTH | BOTTOM, SOUTH | TOP, SOUTH | BOTTOM | TOP, -1):
        assert call(pss, kinds(1, 0, 0, 0, 0, 0)) == -1, pss
    assert b"TPG_SIDE_SOUTH alone" in lib.tpg_last_error()
    assert call(SOUTH, None) == -1 and call(SOUTH, kinds(1), v=None) == -1
    assert lib.tpg_fill_value_gradient_halos(ptrs, 2, SOUTH, kinds(1), vals, None, dy, 0.5, 0.5, *ok, F64, None) == -1
    assert call(BOTTOM, kinds(0, 0, 0, 0, 0, 3)) == -1                                  # unknown kind, even on a side not in the pass
    assert b"unknown kind" in lib.tpg_last_error()
    assert call(SOUTH, kinds(1, 0, 0, 0, 0, 0), d=None) == -1                            # south kind without dy_cf
    assert b"dy_cf" in lib.tpg_last_error()
    assert call(SOUTH, kinds(1, 0, 0, 0, 0, 0), d=C.c_void_p((3 << 20) + 4)) == -1       # dy_cf off its alignment
    assert call(TOP, kinds(0, 0, 2, 0, 0, 0), p=(C.c_void_p * 2)(1 << 20, (2 << 20) + 4)) == -1    # a Float64 field 4-B aligned
    assert call(TOP, kinds(0, 0, 2, 0, 0, 0), c=conds(0, 0, (4 << 20) + 2), ft=F32) == -1          # a condition off its alignment
    assert b"condition pointer" in lib.tpg_last_error()
    assert call(SOUTH, kinds(2, 0, 0, 0, 0, 0), geom=(16, 1, 4, 4, 1, 4)) == -5          # Ny < 2: row 1 is the zipper's row Ny
    assert b"Ny >= 2" in lib.tpg_last_error()
    assert call(SOUTH, kinds(0, 1, 2, 0, 2, 1), geom=(16, 1, 4, 4, 1, 4)) == 0           # no south kind: nothing to do in a south pass
    assert call(BOTTOM | TOP, kinds(1, 0, 0, 1, 0, 0)) == 0                              # no z kind in a z pass
    assert call(TOP, kinds(0, 1, 0, 0, 1, 0)) == 0                                       # bottom kinds are not in a TOP pass
    assert call(BOTTOM | TOP, kinds(0, 1, 2, 0, 2, 1), geom=(16, 12, 4, 4, 4, 0)) == 0   # no z halo: a no-op
    assert call(SOUTH, kinds(1, 0, 0, 2, 0, 0), geom=(16, 12, 4, 4, 0, 4)) == 0          # no y halo: a no-op
    assert call(SOUTH, kinds(1, 0, 0, 0, 0, 0), geom=(15, 12, 4, 4, 4, 4)) == -2         # the geometry checks of every fill
    assert lib.tpg_fill_value_gradient_halos(ptrs, 0, SOUTH, kinds(1), vals, conds(), dy, 0.5, 0.5, *ok, F64, None) == -1


def test_boundary_z_spacings(osg):
    from orthogonalsphericalshellgrids.jl_amd.grids import boundary_z_spacings
    g = vg_grid(osg, z=(-4000, 0), size=(16, 12, 75))
    assert boundary_z_spacings(g) == ((0 - -4000) / 75,) * 2
    assert boundary_z_spacings(g, torch.float32) == (float(np.float32(4000 / 75)),) * 2
    faces = [-100.0, -60.0, -30.0, -10.0, 0.0]
    g = vg_grid(osg, z=faces, size=(16, 12, 4))
    # centres: halo below -120, -80, -45, -20, -5, halo above 5 (faces extrapolated by the end spacings)
    assert boundary_z_spacings(g) == (-80.0 - -120.0, 5.0 - -5.0)
    f = np.array([0.0, 0.1, 0.3, 0.7])
    g = vg_grid(osg, z=torch.from_numpy(f), size=(16, 12, 3), dtype=torch.float32)
    lo, hi = f[0] - (f[1] - f[0]), f[-1] + (f[-1] - f[-2])
    want = (np.float32(0.5 * (f[0] + f[1]) - 0.5 * (lo + f[0])), np.float32(0.5 * (f[-1] + hi) - 0.5 * (f[-2] + f[-1])))
    assert boundary_z_spacings(g) == tuple(float(w) for w in want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_physics(oracle, dtype):
    """on the 60 x 30 grid's own dy_cf: the boundary value is the mean of the two cells about the face and the gradient their difference
    over the spacing, within a few ulps"""
    size, halo = (60, 30, 6), (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    dy_row = oracle.build_grid(size, halo=halo)["dy_cf"][Hy].astype(dtype)
    assert dy_row.min() > 0
    rng = np.random.default_rng(5)
    eps = np.finfo(dtype).eps
    dz = (dtype(12.5), dtype(3.0))
    for kind in (VALUE, GRADIENT):
        mag = 1.0 if kind == VALUE else 1e-5
        a = random_field(rng, size, halo, dtype) + dtype(2)
        sv = rng.uniform(-1, 1, (Nz, Nx + 2 * Hx)).astype(dtype) * dtype(mag)
        bv = rng.uniform(-1, 1, (Ny + 2 * Hy, Nx + 2 * Hx)).astype(dtype) * dtype(mag)
        tv = np.asarray(0.25 * mag, dtype=dtype)
        south_vg(a, size, halo, kind, sv, dy_row)
        z_vg(a, size, halo, (kind, bv), (kind, tv), dz)
        pairs = [(a[Hz:Hz + Nz, Hy - 1], a[Hz:Hz + Nz, Hy], sv, dy_row[None, :]), (a[Hz - 1], a[Hz], bv, dz[0]),
                 (a[Hz + Nz], a[Hz + Nz - 1], tv, dz[1])]
        for side, (c0, c1, v, d) in enumerate(pairs):
            c0, c1, d = c0.astype(np.float64), c1.astype(np.float64), np.float64(1) * d
            scale = np.abs(c0) + np.abs(c1)
            if kind == VALUE:
                assert np.all(np.abs((c0 + c1) / 2 - v) <= 8 * eps * scale), side
            else:
                sgn = 1 if side == 2 else -1          # top: (c^{N+1} - c^N) / dz = g; south / bottom: (c^1 - c^0) / d = g
                assert np.all(np.abs(sgn * (c0 - c1) / d - v) <= 8 * eps * scale / d), side
        # rows j <= -1 and planes beyond the first halo point are untouched
        b = random_field(np.random.default_rng(9), size, halo, dtype)
        keep = b.copy()
        south_vg(b, size, halo, kind, sv, dy_row)
        z_vg(b, size, halo, (kind, bv), (kind, tv), dz)
        changed = b != keep
        assert changed[Hz:Hz + Nz, Hy - 1].all() and changed[Hz - 1].all() and changed[Hz + Nz].all()
        changed[Hz:Hz + Nz, Hy - 1] = changed[Hz - 1] = changed[Hz + Nz] = False
        assert not changed.any()
