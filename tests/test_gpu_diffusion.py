"""GPU tests of the explicit diffusive tendency (tpg_diffusive_tendency, libtripolar_hip_diffusion.so): bit for bit against
tests/diffusion_ref.py on WHOLE parents -- no tolerance anywhere.  G starts as a sentinel (WRITE) or random (ADD), so its halos must come back
as they were; the inputs must come back unchanged.  NaN sits in every cell the header says is not read: the corners and the z-halo planes of
c (all of its halos without the horizontal group), the halos of the flux planes and of a FIELD kappa, the kappa faces 1 and Nz + 1, dz_f[1]
and dz_f[Nz+1], the south halo of the bottom height behind the wall.

The shapes are the smallest at which each path can go wrong (CASES): the smallest grid, Nz = 1, 2, 3, Nx = Hx, Ny = Hy, one chunk per row,
a row count that the rows per item do not divide, and a width that puts a wave's edge and the periodic seam inside a row; and one
Float32 parent past 2^31 elements, where an offset held in 32 bits would wrap."""
import itertools

import numpy as np
import pytest
import torch

import diffusion_ref as R
import special_values as sv
from diffusion_cases import F32, F64, draw
from gpu_harness import _assert_parent, _dev, _free_hbm, _id  # noqa: F401

pytestmark = pytest.mark.gpu

SMALLEST = ((2, 1, 1), (1, 1, 1))
MAIN = ((20, 13, 5), (4, 4, 4))                                    # an odd row count, more levels than twice the look-ahead
SHAPES = [SMALLEST,
          ((2, 1, 2), (1, 1, 1)), ((4, 2, 3), (1, 1, 1)),          # Nz = 2, 3; one chunk per row in Float32
          ((4, 6, 3), (4, 2, 1)),                                  # Nx = Hx
          ((8, 3, 2), (2, 3, 2)),                                  # Ny = Hy, an odd row count
          ((20, 12, 3), (3, 2, 1)),                                # odd Hx: the element-aligned chunks
          MAIN,
          ((130, 5, 2), (4, 4, 4)),                                # 65 chunks per row: a wave's edge and the periodic seam inside a row; 8-B chunks in Float32
          ((48, 40, 6), (5, 5, 5))]                                # the model halo
TERMS = {"h": R.HORIZONTAL, "v": R.VERTICAL, "hv": R.HORIZONTAL | R.VERTICAL, "flux": 0}
FORMS = {"constant": R.CONSTANT, "profile": R.PROFILE, "field": R.FIELD}
BOTTOMS = {"neither": (False, False), "counts": (True, False), "h": (False, True), "both": (True, True)}


def _nan_where_not_read(p):
    """NaN in the cells of c the header says are not read: the corners and the z-halo planes, or every halo cell without the horizontal group"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    keep = np.zeros(p["c"][0].shape, dtype=bool)
    keep[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = True
    if p["terms"] & R.HORIZONTAL:
        keep[Hz:Hz + Nz, Hy:Hy + Ny, Hx - 1:Hx + Nx + 1] = True
        keep[Hz:Hz + Nz, Hy - 1:Hy + Ny + 1, Hx:Hx + Nx] = True
    p["c"] = [np.where(keep, c, np.nan).astype(c.dtype) for c in p["c"]]
    return p


def _problem(case, dtype, **kw):
    size, halo = case
    return _nan_where_not_read(draw(size, halo, dtype, **kw))


def _tendency(osg, gpu, p, offset=0):
    """the status-checked entry point on device copies of the problem p -> the whole G parents on the host; the inputs must be unchanged"""
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    L = osg._lib
    dev = lambda a: None if a is None else _dev(a, gpu, offset)    # noqa: E731
    dtype = p["c"][0].dtype.type
    cs, Gs = [dev(a) for a in p["c"]], [dev(a) for a in p["G"]]
    tables = {}
    for side in ("top", "bottom"):
        planes = p[side]
        tables[side] = None if planes is None else [dev(a) for a in planes]
    form = p["form"]
    kappa = None if form == R.CONSTANT else dev(np.asarray(p["kappa_z"], dtype=dtype))
    horizontal = p["terms"] & R.HORIZONTAL
    m = {k: dev(p[k]) if horizontal else None for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf")}
    az, dz_c = dev(p["az"]), dev(p["dz_c"])
    dz_f = dev(p["dz_f"]) if p["terms"] & R.VERTICAL else None
    counts = None if p["counts"] is None else _dev(np.ascontiguousarray(p["counts"], dtype=np.int32), gpu)
    h, zc = dev(p["h"]), dev(p["zc"])
    ptr = lambda t: None if t is None else t.data_ptr()            # noqa: E731
    table = lambda ts: None if ts is None else (L.C.c_void_p * len(ts))(*[ptr(t) for t in ts])       # noqa: E731
    status = D.diffusion_lib().tpg_diffusive_tendency(
        L.ptr_table(cs), L.ptr_table(Gs), len(cs), p["terms"], p["mode"], p["kappa_h"], ptr(kappa), p["kappa_z"] if form == R.CONSTANT else 0.0, form,
        table(tables["top"]), table(tables["bottom"]), ptr(m["dx_fc"]), ptr(m["dy_fc"]), ptr(m["dx_cf"]), ptr(m["dy_cf"]), ptr(az), ptr(dz_c),
        ptr(dz_f), ptr(counts), p["mask_value"], ptr(h), ptr(zc), int(p["wall"]), *p["size"], *p["halo"], L.ft_of(cs[0].dtype),
        L.current_stream_ptr(gpu))
    D.check_diffusion(status)
    torch.cuda.synchronize()
    for q, (d, a) in enumerate(zip(cs, p["c"])):
        _assert_parent(d.cpu().numpy(), a, ("field unchanged", q))
    if kappa is not None:
        _assert_parent(kappa.cpu().numpy(), np.asarray(p["kappa_z"], dtype=dtype), "kappa unchanged")
    return [g.cpu().numpy() for g in Gs]


def _check(osg, gpu, p, what, offset=0):
    for q, (got, want) in enumerate(zip(_tendency(osg, gpu, p, offset), R.reference(p))):
        _assert_parent(got, want, (what, q))


# ---- the table: every shape in both types, the groups, modes, forms and bottoms crossed in rotation ------------------------------------------------
def _rotation():
    return list(itertools.product(TERMS, (R.ADD, R.WRITE), FORMS, BOTTOMS, ("none", "some", "all")))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: _id((*c, F64))[:-4])
@pytest.mark.parametrize("offset", [0, 1], ids=["16B", "one-element-off"])
def test_whole_parents_are_the_reference_bit_for_bit(osg, gpu, case, dtype, offset):
    every = _rotation()
    start = (SHAPES.index(case) * 37 + offset * 11 + (dtype is F32) * 5) % len(every)
    for n in range(10):                                            # ten combinations per shape, type and alignment, in rotation
        terms, mode, form, bottom, flux = every[(start + 29 * n) % len(every)]
        if flux == "none" and terms == "flux":
            flux = "all"
        masked, closed = BOTTOMS[bottom]
        planes = {"none": ((), ()), "some": ((0,), (1,)), "all": ("all", "all")}[flux]
        p = _problem(case, dtype, nfields=2, terms=TERMS[terms], mode=mode, form=FORMS[form], top=planes[0], bottom_flux=planes[1], masked=masked,
                     closed=closed, seed=n)
        _check(osg, gpu, p, (terms, mode, form, bottom, flux), offset)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", [SMALLEST, MAIN], ids=["smallest", "main"])
def test_every_combination_of_groups_modes_forms_and_bottoms(osg, gpu, case, dtype):
    for terms, mode, form, bottom, flux in _rotation():
        if (flux == "none" and terms == "flux") or (flux == "some" and form != "field"):
            continue
        masked, closed = BOTTOMS[bottom]
        planes = {"none": ((), ()), "some": ((1,), ()), "all": ("all", "all")}[flux]
        p = _problem(case, dtype, nfields=2, terms=TERMS[terms], mode=mode, form=FORMS[form], top=planes[0], bottom_flux=planes[1], masked=masked,
                     closed=closed)
        _check(osg, gpu, p, (terms, mode, form, bottom, flux))


def test_the_drawn_bottom_has_every_kind_of_column_and_face():
    from diffusion_cases import bottom
    (Nx, Ny, Nz), (Hx, Hy, _) = MAIN
    h, zc, counts = bottom(*MAIN, F64)
    n = counts["cc"]
    assert (n[1:, 0] == Nz).all() and (n[:-1, Nx - 1] == Nz).all() and (n[0, 1:3] == Nz).all()        # land at the columns 1 and Nx and in row 1
    assert n[2, 3] == 0 and (n[[1, 3, 2, 2], [3, 3, 2, 4]] == Nz).all()                                 # an isolated wet cell
    assert (n == Nz).any() and (n == Nz - 1).any() and (n == 0).any()
    assert n[Ny - 1, 1] == 0 and (zc <= h[Hy + Ny, Hx + 1]).all()                                       # land at the fold partner of a wet cell of row Ny


# ---- the fields of a call ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("terms", ["hv", "v"])
def test_n_fields_in_one_call_equal_their_one_field_calls(osg, gpu, dtype, terms):
    """n = 1, 2, 3, 4, 5 and 16, flux planes on some of them: the bits do not depend on the grouping"""
    p = _problem(MAIN, dtype, nfields=16, terms=TERMS[terms], mode=R.ADD, form=R.FIELD, top=(0, 3, 4, 15), bottom_flux=(1, 3, 14), masked=True, closed=True)
    want = R.reference(p)
    for n in (1, 2, 3, 4, 5, 16):
        sub = dict(p, **{k: p[k][16 - n:] for k in ("c", "G", "top", "bottom")})
        for q, got in zip(range(16 - n, 16), _tendency(osg, gpu, sub)):
            _assert_parent(got, want[q], (n, q))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("loc", ["fc", "cf"])
def test_u_and_v_take_their_own_area_and_count_planes(osg, gpu, dtype, loc):
    """vertical-only calls: wind stress and explicit vertical viscosity on u with az_fc and n_fc, on v with az_cf and n_cf; no dx_* / dy_*
    plane is passed, and every halo of the fields holds NaN"""
    for case in (MAIN, ((20, 12, 3), (3, 0, 0))):                  # and a halo without y and z: every admitted width is accepted
        for terms, top in ((R.VERTICAL, "all"), (0, "all"), (R.VERTICAL, ())):
            size, halo = case
            masked = halo[1] > 0
            p = _nan_where_not_read(draw(size, halo, dtype, terms=terms, mode=R.ADD, form=R.PROFILE, top=top, bottom_flux=(0,), masked=masked, loc=loc))
            _check(osg, gpu, p, (loc, case, terms, top))


# ---- latitude bands ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [(8, 8, 8), (4, 5)], ids=["three-of-8", "Hy-beside-Hy+1"])
def test_latitude_bands_give_the_rows_of_the_global_call(osg, gpu, rows):
    """through the C ABI: each band is the padded rows of the global arrays -- its seam halos hold what an exchange would deliver -- with the
    south wall on the first band only; the kernel has no fold index map, so the last band's row Ny + 1 is the global one"""
    Hy = 4
    size, halo = (20, sum(rows), 4), (4, Hy, 2)
    p = _problem((size, halo), F64, nfields=2, mode=R.ADD, form=R.FIELD, top="all", bottom_flux=(1,), masked=True, closed=True)
    whole = R.reference(p)
    for q, got in enumerate(_tendency(osg, gpu, p)):
        _assert_parent(got, whole[q], ("global", q))
    j0 = 0
    for band, ny in enumerate(rows):
        sl = slice(j0, j0 + ny + 2 * Hy)
        cut2 = lambda a: None if a is None else np.ascontiguousarray(a[sl])            # noqa: E731
        cut3 = lambda a: None if a is None else np.ascontiguousarray(a[:, sl])         # noqa: E731
        b = dict(p, size=(size[0], ny, size[2]), wall=band == 0, c=[cut3(a) for a in p["c"]], G=[cut3(a) for a in p["G"]], kappa_z=cut3(p["kappa_z"]),
                 top=[cut2(a) for a in p["top"]], bottom=[cut2(a) for a in p["bottom"]], counts=np.ascontiguousarray(p["counts"][j0:j0 + ny]),
                 h=cut2(p["h"]), **{k: cut2(p[k]) for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf", "az")})
        for q, got in enumerate(_tendency(osg, gpu, b)):
            _assert_parent(got[:, Hy:Hy + ny], whole[q][:, Hy + j0:Hy + j0 + ny], (band, q))
        j0 += ny


# ---- special values --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("where", ["fields", "fluxes and kappa", "land"])
def test_special_values(osg, gpu, dtype, where):
    """the pool of IEEE special values (signed zeros, subnormals, the extremes, infinities, NaN) in the fields, in the flux planes and kappa;
    and NaN in every cell of c that lies under the bottom, where the select of a closed face and the mask discard it"""
    size, halo = MAIN
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    p = _problem(MAIN, dtype, nfields=2, mode=R.ADD, form=R.FIELD, top="all", bottom_flux="all", masked=True, closed=True)
    pool = sv.pool(dtype)
    inner = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    if where == "fields":
        for q, c in enumerate(p["c"]):
            c = c.copy()
            c[inner] = sv.tiled(np.roll(pool, 3 * q), (Nz, Ny, Nx))
            p["c"][q] = c
    elif where == "fluxes and kappa":
        for side in ("top", "bottom"):
            for q, J in enumerate(p[side]):
                J = J.copy()
                J[inner[1:]] = sv.tiled(np.roll(pool, q + 1), (Ny, Nx))
                p[side][q] = J
        k = p["kappa_z"].copy()
        k[Hz + 1:Hz + Nz, inner[1], inner[2]] = sv.tiled(np.roll(pool, 5), (Nz - 1, Ny, Nx))
        p["kappa_z"] = k
    else:
        land = np.zeros(p["c"][0].shape, dtype=bool)
        land[Hz:Hz + Nz, Hy - 1:Hy + Ny + 1, Hx - 1:Hx + Nx + 1] = R.inactive_planes(p, dtype)
        p["c"] = [np.where(land, np.nan, c).astype(dtype) for c in p["c"]]
        assert land[inner].any() and not land[inner].all()
    want = R.reference(p)
    assert where == "land" or np.isnan(want[0][inner]).any()
    assert np.isfinite(want[0][inner]).any()
    for q, got in enumerate(_tendency(osg, gpu, p)):
        _assert_parent(got, want[q], (where, q))
    if where == "land":                                            # nothing of it reaches a wet cell
        wet = np.arange(Nz)[:, None, None] >= np.clip(p["counts"], 0, Nz)[None]
        assert np.isfinite(want[0][inner][wet]).all()


# ---- the package ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 4), (4, 4, 4), torch.float32)],
                         ids=["48x40x6-h5-f64", "50x40x4-h4-f32"])
def test_the_plan_equals_the_reference_and_replays_in_a_graph(osg, gpu, size, halo, tdt):
    """on a built immersed grid with its own metrics, spacings, counts and bottom height: the plan's G is the reference's, it allocates nothing
    when called, and a captured graph replays the eager bits; u takes a wind stress through its own FluxBoundaryCondition"""
    from gpu_harness import _grid
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = _grid(osg, size, halo, tdt, True)
    g = grid.underlying_grid
    gen = torch.Generator(device=gpu).manual_seed(5)
    plane = lambda: torch.empty((Ny + 2 * Hy, Nx + 2 * Hx), dtype=tdt, device=gpu).uniform_(-1, 1, generator=gen)     # noqa: E731
    heat, stress = plane(), plane()
    periodic = dict(west=osg.PeriodicBoundaryCondition(), east=osg.PeriodicBoundaryCondition())
    T = osg.CenterField(grid, boundary_conditions=osg.FieldBoundaryConditions(top=osg.FluxBoundaryCondition(heat), **periodic))
    S = osg.CenterField(grid)
    u = osg.XFaceField(grid, boundary_conditions=osg.FieldBoundaryConditions(top=osg.FluxBoundaryCondition(stress), bottom=osg.FluxBoundaryCondition(0.125), **periodic))
    GT, GS, Gu = osg.CenterField(grid), osg.CenterField(grid), osg.XFaceField(grid)
    for f in (T, S, u, GT, GS, Gu):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([T, S, u])
    start = [f.data.clone() for f in (GT, GS, Gu)]
    kappa = torch.empty(Nz + 1, dtype=tdt, device=gpu).uniform_(0, 2, generator=gen)
    closure = osg.VerticalScalarDiffusivity(osg.ExplicitTimeDiscretization(), nu=0.25, kappa=kappa)
    tracers = osg.diffusive_tendency_plan([T, S], [GT, GS], horizontal=osg.HorizontalScalarDiffusivity(kappa=0.61), vertical=closure)
    momentum = osg.diffusive_tendency_plan(u, Gu, vertical=closure)
    assert tracers.top_flux[0] is heat and tracers.top_flux[1] is None and tracers.bottom_flux is None
    assert momentum.top_flux[0] is stress and float(momentum.bottom_flux[0][0, 0]) == 0.125

    def step():
        tracers()
        momentum()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before              # the plans allocate nothing when called
    np_t = F64 if tdt == torch.float64 else F32
    host = lambda t: None if t is None else t.cpu().numpy()        # noqa: E731
    metrics = {k: host(g.arrays[k]).astype(np_t) for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf")}
    dz_c = osg.z_center_spacings(grid, tdt).numpy().astype(np_t)
    dz_f = osg.z_all_face_spacings(grid, tdt).numpy().astype(np_t)
    h = host(grid.immersed_boundary.bottom_height.data)[0]
    zc = host(g.z_centers[Hz:Hz + Nz]).astype(np_t)
    pt = R.problem([host(T.data), host(S.data)], [host(start[0]), host(start[1])], R.HORIZONTAL | R.VERTICAL, R.ADD, size, halo, az=host(g.arrays["az_cc"]).astype(np_t),
                   dz_c=dz_c, dz_f=dz_f, kappa_h=0.61, kappa_z=host(kappa), form=R.PROFILE, top=[host(heat), None], bottom=None,
                   counts=host(grid.column_counts["cc"]), h=h, zc=zc, wall=True, **metrics)
    pu = R.problem([host(u.data)], [host(start[2])], R.VERTICAL, R.ADD, size, halo, az=host(g.arrays["az_fc"]).astype(np_t), dz_c=dz_c, dz_f=dz_f,
                   kappa_z=0.25, form=R.CONSTANT, top=[host(stress)], bottom=[np.full(heat.shape, 0.125, np_t)], counts=host(grid.column_counts["fc"]))
    eager = [host(f.data) for f in (GT, GS, Gu)]
    for got, want, what in zip(eager, R.reference(pt) + R.reference(pu), ("T", "S", "u")):
        _assert_parent(got, want, what)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for f, t in zip((GT, GS, Gu), start):
        f.data.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    for f, want, what in zip((GT, GS, Gu), eager, ("T", "S", "u")):
        _assert_parent(host(f.data), want, ("replay", what))
    # the one-shot form writes into new fields
    out = osg.diffusive_tendency([T, S], horizontal=0.61, top_flux=None)
    pw = dict(pt, terms=R.HORIZONTAL, mode=R.WRITE, top=None, G=[np.zeros_like(a) for a in pt["G"]])
    for got, want in zip(out, R.reference(pw)):
        _assert_parent(host(got.data), want, "one-shot")


def test_the_example_steps_agree_eagerly_and_as_a_graph():
    """examples/forced_model_step.py asserts that its eager and replayed steps agree bit for bit"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "forced_model_step.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ---- past 2^31 elements -----------------------------------------------------------------------------------------------------------------------------------
def test_float32_past_2g_elements(osg, gpu):
    """8640 x 4320 x 64, halo 4, Float32: a parent has 2 694 855 168 elements, offset 2^31 falls in padded plane 57 (interior level 54).  Both
    groups, a FIELD kappa (one plane more), a top and a bottom flux plane, the count plane and the bottom height; data drawn on the device,
    G sentinel-filled, WRITE.
    a. every halo cell of G still holds the sentinel, no interior cell does, and the mask value and the tendency both reach the top level;
    b. the same entry point on three plane windows -- contiguous plane slices of the SAME tensors, fresh small outputs, the tables and the
       counts shifted -- equals the big output on the levels whose two z-faces are the column's own: not the window's first level unless it
       is the column's (the bottom flux enters there), not its last unless it is the column's.  The bottom window lies below 2^30, the
       middle one holds the first interior cell at or past 2^31, the top one ends at the highest addresses.  The small-shape tests hold
       that form of the kernel to the reference;
    c. numpy anchor: the reference on a strip of 16 rows around the row that holds offset 2^31, all 64 levels (a column is walked whole),
       equals the big output on the levels of the middle and the top window (NaNs by NaN-ness).
    Prints its wall time and peak device memory; the peak stays under half the card."""
    import tendency_windows as tw
    from gpu_harness import BIG, BIG_HALO, TWO30, TWO31, _assert_only_the_interior_is_written, _bits_of, _budget, _cell_at, _random
    from orthogonalsphericalshellgrids.jl_amd import diffusion as D
    from vorticity_ref import same_bits
    size, halo = BIG, BIG_HALO
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    plane = sy * sx
    shape = (Nz + 2 * Hz, sy, sx)
    assert np.prod(shape, dtype=np.int64) == 2694855168 and TWO31 // plane == 57
    k31, j31, _ = _cell_at(TWO31, size, halo)
    assert k31 + 1 == 54
    windows = {"bottom": (1, 5), "middle": (52, 57), "top": (60, 64)}                  # levels a..b, 1-based
    compared = {"bottom": [1, 2, 3, 4], "middle": [53, 54, 55, 56], "top": [61, 62, 63, 64]}
    L = osg._lib
    lib = D.diffusion_lib()
    ptr = lambda t: None if t is None else t.data_ptr()            # noqa: E731
    KH, TERMS_HV = 0.61, R.HORIZONTAL | R.VERTICAL

    def call(c, G, kappa, top, bottom, m, dz_c, dz_f, counts, h, zc, n, wall=1):
        tables = [L.ptr_table([t]) for t in (c, G, top, bottom)]
        D.check_diffusion(lib.tpg_diffusive_tendency(
            tables[0], tables[1], 1, TERMS_HV, R.WRITE, KH, ptr(kappa), 0.0, R.FIELD, tables[2], tables[3], *(ptr(m[k]) for k in
            ("dx_fc", "dy_fc", "dx_cf", "dy_cf", "az")), ptr(dz_c), ptr(dz_f), ptr(counts), 0.0, ptr(h), ptr(zc), wall, Nx, Ny, n, Hx, Hy, Hz,
            L.TPG_F32, L.current_stream_ptr(gpu)))

    with _budget(gpu, "diffusive tendency"):
        c = _random(gpu, shape, 100, -1.0, 1.0)
        kappa = _random(gpu, (Nz + 1 + 2 * Hz, sy, sx), 101, 0.0, 2.0)
        m = {k: _random(gpu, (sy, sx), 110 + q, 0.5, 2.0) for q, k in enumerate(("dx_fc", "dy_fc", "dx_cf", "dy_cf", "az"))}
        top, bottom = _random(gpu, (sy, sx), 120, -1.0, 1.0), _random(gpu, (sy, sx), 121, -1.0, 1.0)
        dz_c, dz_f = _random(gpu, (Nz,), 130, 0.5, 2.0), _random(gpu, (Nz + 1,), 131, 0.5, 2.0)
        zc = torch.linspace(-1, 0, 2 * Nz + 1, dtype=torch.float64, device=gpu)[1::2].to(torch.float32).contiguous()
        # a padded plane of counts -- 0 in most columns, drawn from 0..Nz in one of eight, Nz in the columns 1..8 of every row -- and the
        # heights that give them: h = zc[n] (1-based) where n > 0, below every centre elsewhere
        gen = torch.Generator(device=gpu).manual_seed(200)
        n_pad = torch.randint(0, Nz + 1, (sy, sx), dtype=torch.int64, device=gpu, generator=gen)
        n_pad = torch.where(torch.randint(0, 8, (sy, sx), device=gpu, generator=gen) == 0, n_pad, torch.zeros_like(n_pad))
        n_pad[:, Hx:Hx + 8] = Nz
        h = torch.where(n_pad > 0, zc[(n_pad - 1).clamp(min=0)], torch.full((sy, sx), -2.0, dtype=torch.float32, device=gpu)).contiguous()
        counts = n_pad[Hy:Hy + Ny, Hx:Hx + Nx].to(torch.int32).contiguous()
        G = torch.full(shape, tw.SENTINEL, dtype=torch.float32, device=gpu)
        call(c, G, kappa, top, bottom, m, dz_c, dz_f, counts, h, zc, Nz)
        torch.cuda.synchronize()
        # a
        _assert_only_the_interior_is_written(G, size, halo)
        mv = _bits_of(0.0, G)
        level = tw._ints(G)[Hz + Nz - 1, Hy:Hy + Ny, Hx:Hx + Nx]
        assert bool((level[:, :8] == mv).all()) and not bool((level[:, 8:] == mv).all())
        # b
        for which, (a, b) in windows.items():
            n = b - a + 1
            cut = c[a - 1:a - 1 + n + 2 * Hz]
            kcut = kappa[a - 1:a - 1 + n + 1 + 2 * Hz]
            wG = torch.full((n + 2 * Hz, sy, sx), tw.SENTINEL, dtype=torch.float32, device=gpu)
            assert cut.is_contiguous() and kcut.is_contiguous() and all(t.data_ptr() % 16 == 0 for t in (cut, kcut, wG, c, G, kappa))
            assert cut.data_ptr() - c.data_ptr() == (a - 1) * plane * 4
            if which == "bottom":
                assert (b + 1 + 2 * Hz) * plane < TWO30
            if which == "top":
                assert (a - 1 + Hz) * plane > TWO31 and b == Nz    # every interior level of the window lies past 2^31
            call(cut, wG, kcut, top, bottom, m, dz_c[a - 1:b], dz_f[a - 1:b + 1], (counts - (a - 1)).contiguous(), h, zc[a - 1:b], n)
            torch.cuda.synchronize()
            for k in compared[which]:
                assert a <= k <= b and (k > a or a == 1) and (k < b or b == Nz)
                assert tw.equal_bits(wG[Hz + k - a], G[Hz + k - 1]), (which, k)
            del cut, kcut, wG
        # c
        lo = min(max(j31 - 8, 1), Ny - 16)
        assert lo <= j31 < lo + 16
        rows = slice(lo, lo + 16 + 2 * Hy)                          # the strip's padded rows: its y-halos are rows of the big interior
        host = lambda t: t[..., rows, :].contiguous().cpu().numpy()    # noqa: E731
        p = R.problem([host(c)], [np.full((Nz + 2 * Hz, 16 + 2 * Hy, sx), tw.SENTINEL, F32)], TERMS_HV, R.WRITE, (Nx, 16, Nz), halo, az=host(m["az"]),
                      dz_c=dz_c.cpu().numpy(), dz_f=dz_f.cpu().numpy(), kappa_h=KH, kappa_z=host(kappa), form=R.FIELD, top=[host(top)], bottom=[host(bottom)],
                      counts=counts[lo:lo + 16].cpu().numpy(), h=host(h), zc=zc.cpu().numpy(), wall=False,
                      **{k: host(m[k]) for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf")})
        want = R.tendency_planes(p, 0)
        for k in compared["middle"] + compared["top"]:
            got = G[Hz + k - 1, Hy + lo:Hy + lo + 16, Hx:Hx + Nx].contiguous().cpu().numpy()
            bad = same_bits(got, want[k - 1])
            assert bad == 0, (k, bad, "cells differ of", got.size)
        del c, G, kappa, m, top, bottom, n_pad, h, counts, p, want
