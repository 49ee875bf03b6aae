"""GPU tests of the grid-fitted immersed boundary: tpg_immersed_column_counts and tpg_mask_immersed_fields, GridFittedBottom /
ImmersedBoundaryGrid, mask_immersed_field / immersed_mask_plan and halo_fill_plan(..., mask_immersed=value).  Bit-exact on the WHOLE
parent against tests/immersed_ref.py (numpy, from the predicate), compared as integers so that NaNs count: the four count planes; the
eight locations with sentinels in every halo cell and NaN in a tenth of the interior cells; the direct C call; the reference's own cases
(test/test_zipper_boundary_conditions.jl:47-54, the bottom of examples/bickley_jet.jl); a property layer at 3600 x 1800 x 75 that needs no
second implementation; the plan with the mask in front of the fill, eager and as a replayed graph; latitude bands through the loop-back
transport."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest
import torch

from bounded_ref import random_field
from immersed_ref import chunk_classes, column_counts, draw_columns, heights_of, inactive_cells, mask_immersed_field

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
KEYS = ("cc", "fc", "cf", "ff")
HALOS = [(4, 4, 4), (5, 5, 5), (3, 2, 1)]
SIZES = [(48, 40, 3), (48, 40, 6), (50, 40, 3)]


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _dev(host, gpu, offset):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return t


def _zc(Nz, dtype):
    return ((np.arange(Nz) + 0.5) / Nz).astype(dtype)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _loc(osg, loc):
    return tuple(osg.Face if b else osg.Center for b in loc)


def _filled_bottom(oracle, hin, size, halo):
    """the padded bottom height after fill_halo_regions (zipper (Center, Center, +1), periodic x), on the host"""
    (Nx, Ny, _), (Hx, Hy, _) = size, halo
    hp = np.zeros((1, Ny + 2 * Hy, Nx + 2 * Hx), dtype=hin.dtype)
    hp[0, Hy:Hy + Ny, Hx:Hx + Nx] = hin
    oracle.fill_halo_regions(hp, 0, 0, 1, (Nx, Ny, 1), (Hx, Hy, 0))
    return hp[0]


@pytest.mark.parametrize("wall", [True, False], ids=["wall", "seam"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("halo", HALOS, ids=["h444", "h555", "h321"])
@pytest.mark.parametrize("size", SIZES, ids=["48x40x3", "48x40x6", "50x40x3"])
def test_count_planes_against_their_definition(osg, gpu, size, halo, dtype, wall):
    """the direct C call on a random padded bottom (halo cells hold heights of their own): the four planes, 16-B aligned and offset by one
    element (bottom, centres and planes alike), equal the definition; the element in front of an offset plane is not written"""
    lib = osg._lib.lib()
    (Nx, Ny, Nz), (Hx, Hy, _) = size, halo
    rng = np.random.default_rng([*size, *halo, int(wall), np.dtype(dtype).itemsize])
    zc = _zc(Nz, dtype)
    h = heights_of(rng.integers(0, Nz + 1, (Ny + 2 * Hy, Nx + 2 * Hx)), zc, rng)
    h[Hy:Hy + Ny, Hx:Hx + Nx] = heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)
    want = column_counts(h, zc, size, halo, wall)
    for offset in (0, 1):
        dh, dz = _dev(h, gpu, offset), _dev(zc, gpu, offset)
        raw = torch.full((4, Ny * Nx + offset), -7, dtype=torch.int32, device=gpu)
        planes = [raw[q, offset:] for q in range(4)]
        assert all(p.data_ptr() % 4 == 0 for p in planes) and (offset == 0 or any(p.data_ptr() % 16 for p in planes))
        osg._lib.check(lib.tpg_immersed_column_counts(dh.data_ptr(), dz.data_ptr(), int(wall), *(p.data_ptr() for p in planes),
                                                      Nx, Ny, Nz, Hx, Hy, osg._lib.ft_of(_tdt(dtype)), osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        for q, key in enumerate(KEYS):
            assert np.array_equal(planes[q].cpu().numpy().reshape(Ny, Nx), want[key]), (key, offset)
        assert offset == 0 or bool((raw[:, 0] == -7).all())
        # one plane alone: the others NULL
        alone = torch.full((Ny * Nx,), -7, dtype=torch.int32, device=gpu)
        osg._lib.check(lib.tpg_immersed_column_counts(dh.data_ptr(), dz.data_ptr(), int(wall), None, None, None, alone.data_ptr(),
                                                      Nx, Ny, Nz, Hx, Hy, osg._lib.ft_of(_tdt(dtype)), osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        assert np.array_equal(alone.cpu().numpy().reshape(Ny, Nx), want["ff"])


@pytest.mark.parametrize("value", [0.0, 0.1], ids=["zero", "tenth"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("size,halo", [(s, h) for s in SIZES for h in HALOS],
                         ids=lambda v: "x".join(map(str, v)))
def test_mask_is_bit_exact_at_the_eight_locations(osg, oracle, gpu, size, halo, dtype, offset, value):
    """through the public names: an ImmersedBoundaryGrid from a (Ny, Nx) bottom, 40 fields per z location in ONE plan (two geometry groups,
    three batches each) over the eight locations, every halo cell a sentinel and NaN in a tenth of the interior cells beforehand; the
    filled bottom, the four count planes and the whole parent of every field are compared with the host reference, as integers"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = _tdt(dtype)
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo)
    zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
    assert zc.dtype == dtype
    rng = np.random.default_rng([*size, *halo, offset, np.dtype(dtype).itemsize])
    hin = heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(torch.from_numpy(hin)))
    assert ibg.underlying_grid is grid and ibg.Nx == Nx and osg.is_tripolar(ibg)
    hp = _filled_bottom(oracle, hin, size, halo)
    assert np.array_equal(_bits(ibg.immersed_boundary.bottom_height.data.cpu().numpy()[0]), _bits(hp))
    want_n = column_counts(hp, zc, size, halo, True)
    for key in KEYS:
        assert ibg.column_counts[key].dtype == torch.int32
        assert np.array_equal(ibg.column_counts[key].cpu().numpy(), want_n[key]), key
    # the input holds what it is meant to hold: at every level, chunks of 2 and of 4 columns with no, all and some masked elements
    for W in (2, 4):
        assert all(all(t) for t in chunk_classes(want_n["cc"], Nz, W)), W
    ina = inactive_cells(hp, zc, size, halo, True)
    fields = []
    for zl in (0, 1):
        for q in range(40):
            loc = (q % 2, (q // 2) % 2, zl)
            fsize = (Nx, Ny, Nz + zl)
            host = random_field(rng, fsize, halo, dtype)
            inner = host[Hz:Hz + Nz + zl, Hy:Hy + Ny, Hx:Hx + Nx]
            inner[rng.random(inner.shape) < 0.1] = np.nan
            keep = inner.copy()
            host[...] = SENTINEL
            host[Hz:Hz + Nz + zl, Hy:Hy + Ny, Hx:Hx + Nx] = keep
            fields.append((loc, host, osg.Field(_loc(osg, loc), ibg, data=_dev(host, gpu, offset))))
    plan = osg.immersed_mask_plan([f for *_, f in fields], value)
    assert len(plan._steps) == 2 and all(len(calls) == 1 and calls[0][1][1] == 40 for _, calls in plan._steps)
    plan()
    torch.cuda.synchronize()
    for loc, host, f in fields:
        want, per = mask_immersed_field(host, loc, value, hp, zc, size, halo, True, ina)
        assert np.array_equal(_bits(f.data.cpu().numpy()), _bits(want)), loc
        assert 0 < per.sum() < per.size


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_direct_call_changes_only_the_documented_cells(osg, gpu, ft):
    """the C call alone on sentinel-filled parents with count planes of its own: rows of 2 (Float32: 8-B chunks), 4, 6, 8 and 16, offset
    pointers, no halo in x, y or z, z-Center and z-Face fields with different values in one table, a one-level z-Face field (nothing to
    write): exactly the cells k <= n (k <= min(n + 1, Nz - 1)) of the interior change"""
    lib = osg._lib.lib()
    dtype, code = (np.float32, osg._lib.TPG_F32) if ft == "f32" else (np.float64, osg._lib.TPG_F64)
    for (size, halo), offset in itertools.product((((2, 6, 2), (0, 2, 1)), ((4, 6, 2), (1, 2, 2)), ((6, 5, 3), (2, 2, 0)), ((6, 5, 2), (2, 0, 1)),
                                                   ((16, 7, 4), (4, 3, 2)), ((8, 4, 1), (1, 1, 1)), ((12, 3, 5), (4, 1, 1))), (0, 1)):
        (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
        rng = np.random.default_rng(13)
        table = [(0, dtype(0)), (1, dtype(-2.5)), (0, dtype(0.1)), (1, dtype(0))]
        ns = [rng.integers(0, Nz + 1 - zl, (Ny, Nx)).astype(np.int32) for zl, _ in table]
        raw = [torch.empty(Ny * Nx + offset, dtype=torch.int32, device=gpu) for _ in table]
        planes = [r[offset:] for r in raw]
        for p, n in zip(planes, ns):
            p.copy_(torch.from_numpy(n.reshape(-1)))
        hosts = [np.full((Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), SENTINEL, dtype=dtype) for _ in table]
        devs = [_dev(h, gpu, offset) for h in hosts]
        k = len(table)
        osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table(devs), k, osg._lib.ptr_table(planes), (C.c_int8 * k)(*[zl for zl, _ in table]),
                                                    (C.c_double * k)(*[float(v) for _, v in table]), *size, *halo, code,
                                                    osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        lev = np.arange(1, Nz + 1)[:, None, None]
        for (zl, v), n, host, dev in zip(table, ns, hosts, devs):
            per = lev <= (np.minimum(n + 1, Nz - 1) if zl else n)[None]
            want = host.copy()
            inner = want[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
            inner[per] = v
            got = dev.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (size, halo, offset, zl)
            assert (got != SENTINEL).sum() == per.sum(), (size, halo, offset, zl)


def test_reference_zipper_case_random_bottom_is_mirror_symmetric(osg, oracle, gpu):
    """test/test_zipper_boundary_conditions.jl:47-54: TripolarGrid(size = (10, 10, 1)), GridFittedBottom(rand): row Ny of bottom_height is
    mirror-symmetric; and c, u masked on that grid equal the host reference"""
    size, halo = (10, 10, 1), (4, 4, 4)
    torch.manual_seed(7)
    grid = osg.TripolarGrid(osg.GPU(0), size=size)
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(lambda lam, phi: torch.rand_like(lam)))
    bottom_height = ibg.immersed_boundary.bottom_height
    inner = osg.interior(bottom_height)
    assert inner.shape == (1, 10, 10) and torch.equal(inner[0, 9, :], inner[0, 9, :].flip(0))
    hp = bottom_height.data.cpu().numpy()[0]
    zc = grid.z_centers[4:5].cpu().numpy()
    want_n = column_counts(hp, zc, size, halo, True)
    assert 0 < want_n["cc"].sum() < 100
    rng = np.random.default_rng(3)
    for loc in ((0, 0, 0), (1, 0, 0)):
        host = random_field(rng, size, halo, np.float64)
        f = osg.Field(_loc(osg, loc), ibg, data=_dev(host, gpu, 0))
        osg.mask_immersed_field(f)
        want, _ = mask_immersed_field(host, loc, 0.0, hp, zc, size, halo)
        assert np.array_equal(_bits(f.data.cpu().numpy()), _bits(want)), loc
        osg.fill_halo_regions(f)                                   # :56-63: fields on the immersed grid fill as on the bare one
        oracle.fill_halo_regions(want, loc[0], loc[1], -1 if loc[0] else 1, size, halo)
        assert np.array_equal(f.data.cpu().numpy(), want), loc


def test_bickley_bottom_masks_the_pole_boxes_and_the_southern_cap(osg, gpu):
    """examples/bickley_jet.jl:9-29 on this host: 180 x 90 x 1, halo 5, poles at 45 / 225 E, 25 N: the pole boxes and phi < -78 are
    masked, nothing else; (u, v, c) masked and filled"""
    size, halo = (180, 90, 1), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    lp, pp = 45, 25
    grid = osg.TripolarGrid(osg.GPU(0), size=size, halo=halo, first_pole_longitude=lp, north_poles_latitude=pp)
    box = lambda lam, phi: ((((lam - lp).abs() < 5) & ((pp - phi).abs() < 5)) | (((lam - (lp + 180)).abs() < 5) & ((pp - phi).abs() < 5))
                            | (phi < -78))
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(lambda lam, phi: torch.where(box(lam, phi), 1.0, 0.0).to(lam.dtype)))
    want = box(grid.interior("lambda_cc"), grid.interior("phi_cc"))
    cc = ibg.column_counts["cc"]
    assert torch.equal(cc[:Ny - 1] == 1, want[:Ny - 1]) and torch.equal(cc[Ny - 1, :Nx // 2] == 1, want[Ny - 1, :Nx // 2])
    assert torch.equal(cc[Ny - 1], cc[Ny - 1].flip(0))             # row Ny: the fold's substitution made it mirror-symmetric
    assert bool(((cc == 0) | (cc == 1)).all())
    north = want & (grid.interior("phi_cc") > 0)
    assert bool(north.any()) and bool((want & ~north).any()) and int(cc.sum()) < Nx * Ny // 8
    gen = torch.Generator(device=gpu).manual_seed(1)
    u, v, c = osg.XFaceField(ibg), osg.YFaceField(ibg), osg.CenterField(ibg)
    for f in (u, v, c):
        f.data.uniform_(0.5, 1.5, generator=gen)
    osg.mask_immersed_field([u, v, c])
    n = ibg.column_counts
    for f, key in ((u, "fc"), (v, "cf"), (c, "cc")):
        assert torch.equal(osg.interior(f)[0] == 0, n[key] == 1), key
    osg.fill_halo_regions([u, v, c])
    assert torch.equal(osg.interior(c)[0] == 0, n["cc"] == 1)


def _property_bottom(lam, phi):
    """a bottom that is a function of (lambda, phi) only: about half of the cells of z = (-1, 0) masked, pole boxes and southern cap land"""
    rl, rp = torch.deg2rad(lam), torch.deg2rad(phi)
    h = -(0.5 + 0.5 * torch.sin(3 * rl) * torch.cos(2 * rp) + 0.2 * torch.cos(5 * rl) * torch.sin(4 * rp)).clamp(0, 1)
    land = (((lam - 70).abs() < 5) & ((55 - phi).abs() < 5)) | (((lam - 250).abs() < 5) & ((55 - phi).abs() < 5)) | (phi < -78)
    return torch.where(land, torch.zeros_like(h), h)


@pytest.mark.parametrize("h,tdt", [(4, torch.float64), (5, torch.float32)], ids=["halo4-f64", "halo5-f32"])
def test_properties_at_the_headline_size(osg, gpu, h, tdt):
    """3600 x 1800 x 75, no second implementation in the loop, for c, u, v, zeta: the mask writes 0 to the cells k <= n of the interior
    and changes nothing else on the whole parent; it is idempotent; and THE FILL NEVER UNMASKS: on the interior mask(fill(mask(f))) ==
    fill(mask(f)), compared as numbers on NaN-free input (the fold of a masked source with sign -1 leaves -0.0 where the mask writes +0.0)"""
    size, halo = (3600, 1800, 75), (h, h, h)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(_property_bottom))
    lev = torch.arange(1, Nz + 1, device=gpu, dtype=torch.int32)[:, None, None]
    gen = torch.Generator(device=gpu).manual_seed(11)
    for loc, key in (((0, 0, 0), "cc"), ((1, 0, 0), "fc"), ((0, 1, 0), "cf"), ((1, 1, 0), "ff")):
        n = ibg.column_counts[key]
        per = lev <= n[None]
        frac = float(per.float().mean())
        assert 0.3 < frac < 0.8, (key, frac)
        f = osg.Field(_loc(osg, loc), ibg)
        f.data.uniform_(0.5, 1.5, generator=gen)
        want = f.data.clone()
        want[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(per, 0)
        plan = osg.immersed_mask_plan(f)
        plan()
        assert torch.equal(f.data, want), ("masked cells only", key)
        plan()
        assert torch.equal(f.data, want), ("idempotent", key)
        del want
        osg.fill_halo_regions(f)
        filled = osg.interior(f).clone()
        assert bool(((filled == 0) | ~per).all()), ("the fill never unmasks", key)
        plan()
        assert bool((osg.interior(f) == filled).all()), ("mask(fill(mask)) == fill(mask)", key)
        del f, filled, per, plan
        gc.collect()
        torch.cuda.empty_cache()


def _model_fields(osg, grid, gpu, tdt, seed, w_bottom):
    nf, per = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition
    imp = osg.ImpenetrableBoundaryCondition
    Ce, Fa = osg.Center, osg.Face
    specs = [("u", (Fa, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())), ("v", (Ce, Fa, Ce), dict(south=imp(), bottom=nf(), top=nf())),
             ("w", (Ce, Ce, Fa), dict(south=nf(), bottom=w_bottom, top=imp())), ("T", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())),
             ("S", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf()))]
    gen = torch.Generator(device=gpu).manual_seed(seed)
    out = []
    for name, loc, sides in specs:
        f = osg.Field(loc, grid, name=name, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))
        f.data.uniform_(0.5, 1.5, generator=gen)
        out.append(f)
    return out


@pytest.mark.parametrize("h,tdt", [(4, torch.float64), (5, torch.float64), (5, torch.float32)], ids=["halo4-f64", "halo5-f64", "halo5-f32"])
def test_plan_with_the_mask_in_front_equals_mask_then_fill(osg, gpu, h, tdt):
    """halo_fill_plan(fields, mask_immersed=0.0) on a model's (u, v, w, T, S) with its default conditions (w's bottom Open with a value, to
    show the order): the mask launch is the first call of every geometry group, and the plan -- eager, and captured and replayed as a
    graph -- leaves every parent bit-identical to mask_immersed_field followed by the plain plan"""
    size, halo = (128, 48, 6), (h, h, h)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
    zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
    rng = np.random.default_rng(19)
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)))
    bottom = osg.OpenBoundaryCondition(0.5)
    a, b, c = (_model_fields(osg, ibg, gpu, tdt, 23, bottom) for _ in range(3))
    start = [f.data.clone() for f in c]
    osg.mask_immersed_field(a)
    plain = osg.halo_fill_plan(a)
    assert not any(fn.__name__ == "tpg_mask_immersed_fields" for _, calls, _ in plain._steps for fn, *_ in calls)
    plain()
    plan = osg.halo_fill_plan(b, mask_immersed=0.0)
    assert [[fn.__name__ for fn, *_ in calls][:2] for _, calls, _ in plan._steps] == [["tpg_mask_immersed_fields", "tpg_fill_open_faces"]] * 2
    plan()
    graph = osg.halo_fill_plan(c, mask_immersed=0.0).graph()      # graph() runs the plan once eagerly before it captures
    for f, s in zip(c, start):
        f.data.copy_(s)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for fa, fb, fc in zip(a, b, c):
        assert torch.equal(fa.data.view(torch.int64 if tdt == torch.float64 else torch.int32),
                           fb.data.view(torch.int64 if tdt == torch.float64 else torch.int32)), fa.name
        assert torch.equal(fb.data, fc.data), fa.name
    w, T = b[2], b[3]
    assert bool((w.data[Hz, Hy:Hy + Ny - 1, Hx:Hx + Nx] == 0.5).all())     # the Open bottom value overwrote the mask's 0 at k = 1
    assert torch.equal(osg.interior(T)[0] == 0, ibg.column_counts["cc"] >= 1)
    # a grid without an immersed boundary: the option is a no-op, as Oceananigans' method is
    bare = osg.halo_fill_plan(_model_fields(osg, grid, gpu, tdt, 23, bottom), mask_immersed=0.0)
    assert not any(fn.__name__ == "tpg_mask_immersed_fields" for _, calls, _ in bare._steps for fn, *_ in calls)
    with pytest.raises(NotImplementedError, match="reduced and z-windowed"):
        osg.mask_immersed_field(osg.Field((osg.Center, osg.Center, None), ibg))
    with pytest.raises(NotImplementedError, match="reduced and z-windowed"):
        osg.mask_immersed_field(osg.Field((osg.Center, osg.Center, osg.Center), ibg, indices=(slice(None), slice(None), Nz)))


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("halo", [(4, 4, 2), (5, 5, 5)], ids=["halo442", "halo5"])
def test_bands_with_loopback_transport(osg, gpu, R, halo):
    """latitude bands: every rank's bottom (seam halo rows included), count planes and masked interiors equal the rows of the serial
    ones; halo cells of the band fields are not touched; the south wall is rank 0's only"""
    size = (48, 36, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(31)
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo)
    zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
    hin = torch.from_numpy(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)).to(gpu)
    serial = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(hin))
    locs = list(itertools.product((0, 1), repeat=3))
    globs = [torch.from_numpy(random_field(rng, (Nx, Ny, Nz + loc[2]), halo, np.float64)).to(gpu) for loc in locs]
    sfields = [osg.Field(_loc(osg, loc), serial, data=g.clone()) for loc, g in zip(locs, globs)]
    osg.mask_immersed_field(sfields, 0.25)
    mailbox = osg.LoopbackMailbox()
    bands = []
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r)
        bg = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)
        jstart, jend = bg.jrange
        bands.append(osg.ImmersedBoundaryGrid(bg, osg.GridFittedBottom(hin[jstart - 1:jend]), exchange=mailbox.endpoint(r)))
    with pytest.raises(RuntimeError, match="finish"):
        bands[0].column_counts
    for ibg in bands:                                              # every rank has posted: delivery and the count planes
        ibg.finish()
    hs = serial.immersed_boundary.bottom_height.data
    for r, ibg in enumerate(bands):
        jstart, jend = ibg.jrange
        rows = slice(jstart - 1, jend + 2 * Hy)
        hb = ibg.immersed_boundary.bottom_height.data
        lo = Hy if r == 0 else 0                                   # rank 0's south halo rows are nobody's
        assert torch.equal(hb[:, lo:], hs[:, rows][:, lo:]), r
        for key in KEYS:
            assert torch.equal(ibg.column_counts[key], serial.column_counts[key][jstart - 1:jend]), (r, key)
        fs = [osg.Field(_loc(osg, loc), ibg, data=g[:, rows].contiguous()) for loc, g in zip(locs, globs)]
        osg.mask_immersed_field(fs, 0.25)
        for f, s, g in zip(fs, sfields, globs):
            assert torch.equal(osg.interior(f), osg.interior(s)[:, jstart - 1:jend]), (r, f.loc)
            untouched = g[:, rows].clone()
            untouched[Hz:Hz + f.Nz, Hy:Hy + f.Ny, Hx:Hx + Nx] = osg.interior(f)
            assert torch.equal(f.data, untouched), (r, f.loc)
