"""GPU tests of the vertical vorticity at (Face, Face, Center): tpg_vertical_vorticity through the C ABI, and vertical_vorticity /
vorticity_plan / VerticalVorticityField / compute_ through the package.  Compared BIT FOR BIT with tests/vorticity_ref.py (numpy in the
fields' type: every operation of the rule is one correctly rounded IEEE operation, so the reference is exact and there is no tolerance
anywhere in this file); NaNs compare by NaN-ness; no case and no cell is left out of a comparison.

Shapes: the smallest at which each path can go wrong -- the reference's own test size; the minimum halo (every read touches the halo's last
cell); rows off the 16-B grid with an odd Hx (the element-aligned chunks); the model halo 5; Float32 with Nx = 2 mod 4 (8-B chunks); one
shape with more work items than resident threads and Ny no multiple of the rows an item owns (tile edges, the last partial tile); and one
case past 2^31 elements."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_harness import _assert_parent, _dev, _free_hbm, _id  # noqa: F401
from immersed_ref import column_counts, draw_columns, heights_of, inactive_cells, peripheral
from special_values import pool
from vorticity_ref import cells_read, interior_vorticity, vertical_vorticity

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#         size            halo       element type
TABLE = [((10, 10, 1), (4, 4, 4), F64),            # the reference's own test size
         ((20, 12, 3), (1, 1, 1), F64),            # the minimum halo: every read touches the halo's last cell
         ((20, 12, 3), (1, 1, 1), F32),
         ((20, 12, 3), (3, 2, 1), F64),            # rows off the 16-B grid, odd Hx: the element-aligned chunks
         ((48, 40, 6), (5, 5, 5), F64),            # the model halo
         ((48, 40, 6), (5, 5, 5), F32),
         ((50, 40, 3), (4, 4, 4), F32),            # Nx = 2 mod 4: 8-B chunks
         ((2304, 1283, 1), (4, 4, 4), F64)]        # 321 row tiles x 1152 chunks = 369 792 items in 1445 blocks, more than are resident
#                                                    (256 CUs x 5); 1283 = 320 * 4 + 3: the last tile has 3 rows
SENTINEL = 12345.0
MASK_VALUE = 0.1                                   # not representable: converted once to the field type


def _tdt(dtype):
    return torch.float64 if dtype == F64 else torch.float32


def _shapes(size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)


_CASES = {}


def _case(case):
    """host arrays of a case, random in EVERY cell (halos included), and the reference parent of zeta from a sentinel-filled one: computed
    once per case, shared by the tests, never modified (tests copy what they change)"""
    if case not in _CASES:
        size, halo, dtype = case
        parent, plane = _shapes(size, halo)
        rng = np.random.default_rng([*size, *halo, np.dtype(dtype).itemsize])
        h = {"u": rng.uniform(-1, 1, parent).astype(dtype), "v": rng.uniform(-1, 1, parent).astype(dtype),
             "dx_fc": rng.uniform(0.5, 2, plane).astype(dtype), "dy_cf": rng.uniform(0.5, 2, plane).astype(dtype),
             "az_ff": rng.uniform(0.5, 2, plane).astype(dtype)}
        h["zeta0"] = np.full(parent, SENTINEL, dtype)
        h["want"] = _ref(h, size, halo)
        for a in h.values():
            a.setflags(write=False)
        _CASES[case] = h
    return _CASES[case]


def _ref(h, size, halo, n_ff=None, value=0.0):
    zeta0 = np.full(h["u"].shape, SENTINEL, h["u"].dtype)
    return vertical_vorticity(h["u"], h["v"], zeta0, h["dx_fc"], h["dy_cf"], h["az_ff"], size, halo, n_ff, value)


def _call(osg, gpu, d, size, halo, n_ff=None, value=0.0, zeta=None):
    """tpg_vertical_vorticity on the device arrays d -> the whole parent of zeta on the host"""
    lib = osg._lib.operators_lib()
    z = d["zeta"] if zeta is None else zeta
    osg._lib.check_operators(lib.tpg_vertical_vorticity(d["u"].data_ptr(), d["v"].data_ptr(), z.data_ptr(), d["dx_fc"].data_ptr(), d["dy_cf"].data_ptr(),
                                              d["az_ff"].data_ptr(), None if n_ff is None else n_ff.data_ptr(), value, *size, *halo,
                                              osg._lib.ft_of(d["u"].dtype), osg._lib.current_stream_ptr(gpu)))
    return z.cpu().numpy()


def _device(h, gpu, offset=0):
    d = {k: _dev(h[k], gpu, offset) for k in ("u", "v", "dx_fc", "dy_cf", "az_ff")}
    d["zeta"] = _dev(np.full(h["u"].shape, SENTINEL, h["u"].dtype), gpu, offset)
    return d


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_interior_is_bit_exact_and_no_halo_cell_of_zeta_is_written(osg, gpu, case, offset):
    """random data in every cell, zeta's parent pre-filled with a sentinel: the whole parent equals the reference's -- the interior the
    rule, every halo cell still the sentinel -- with every pointer on the 16-B grid and with every pointer one element past an allocation"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    got = _call(osg, gpu, _device(h, gpu, offset), size, halo)
    _assert_parent(got, h["want"], "parent")
    halo_cells = np.ones(got.shape, bool)
    halo_cells[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
    assert (got[halo_cells] == SENTINEL).all() and not (got[~halo_cells] == SENTINEL).any()


@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_no_cell_outside_the_stencil_is_read(osg, gpu, case):
    """every cell of u, v and the metrics that the rule does not read is NaN: the result has no NaN and equals the clean one"""
    size, halo, dtype = case
    h = _case(case)
    read = cells_read(size, halo)
    poisoned = {k: np.where(read[k], h[k], dtype(np.nan)) for k in read}
    assert all(np.isnan(poisoned[k]).sum() == (~read[k]).sum() for k in read) and np.isnan(poisoned["u"]).any()
    got = _call(osg, gpu, _device(poisoned, gpu), size, halo)
    assert not np.isnan(got).any()
    _assert_parent(got, h["want"], "poisoned")


@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_special_values_in_read_cells(osg, gpu, case):
    """+-0, subnormals, +-Inf, NaN, +-max (overflowing products and differences) planted in about a third of the cells of u, v, dx_fc and
    dy_cf, and a tenth of az_ff (az_ff = +-0 among them: x / 0): bit for bit numpy's, which computes the same IEEE operations"""
    size, halo, dtype = case
    h = _case(case)
    rng = np.random.default_rng([7, *size, *halo])
    p = pool(dtype)
    planted = {}
    for name, share in (("u", 0.3), ("v", 0.3), ("dx_fc", 0.3), ("dy_cf", 0.3), ("az_ff", 0.1)):
        a = h[name].copy()
        where = rng.random(a.shape) < share
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
        planted[name] = a
    with np.errstate(all="ignore"):
        want = _ref(planted, size, halo)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    inner = want[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert np.isnan(inner).any() and np.isfinite(inner).any() and (np.isinf(inner).any() or inner.size < 1000)
    got = _call(osg, gpu, _device(planted, gpu), size, halo)
    _assert_parent(got, want, "special values")


_PLANES = {}


def _count_plane(case):
    """the (Face, Face) count plane for a drawn bottom (land columns, open columns, everything between), from the PREDICATE of
    tests/immersed_ref.py: the peripheral (Face, Face, Center) nodes of a padded bottom height whose halos continue it (periodic in x, the
    edge rows in y), south wall; the masked levels of a column are a prefix, so their number is the plane.  Checked against the plane's own
    definition (column_counts, a Python loop) on the small cases.  Computed once per case."""
    if case in _PLANES:
        return _PLANES[case]
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng([11, *size, *halo])
    zc = ((np.arange(Nz) + 0.5) / Nz).astype(dtype)
    hin = heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)
    hp = np.pad(np.pad(hin, ((0, 0), (Hx, Hx)), mode="wrap"), ((Hy, Hy), (0, 0)), mode="edge")
    per = peripheral(inactive_cells(hp, zc, size, halo, True), (1, 1, 0), size)
    n = per.sum(0).astype(np.int32)
    assert np.array_equal(per, np.arange(1, Nz + 1)[:, None, None] <= n[None])           # a prefix of the column
    if Nx * Ny < 5000:
        assert np.array_equal(n, column_counts(hp, zc, size, halo, True)["ff"])
    assert n.shape == (Ny, Nx) and (n == Nz).any() and (n == 0).any()
    n.setflags(write=False)
    _PLANES[case] = n
    return n


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_fused_mask_equals_the_mask_pass_and_reads_nothing_under_it(osg, gpu, case, offset):
    """with a count plane: (1) the reference with the mask; (2) the unmasked call followed by tpg_mask_immersed_fields on zeta, bit for
    bit on the whole parent; (3) with every cell of u and v that only masked nodes read turned into NaN, the same bits again"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    n = _count_plane(case)
    want = _ref(h, size, halo, n, MASK_VALUE)
    d = _device(h, gpu, offset)
    nd = _dev(n, gpu, offset)
    got = _call(osg, gpu, d, size, halo, nd, MASK_VALUE)
    _assert_parent(got, want, "fused mask")
    # the two-pass form
    lib = osg._lib.lib()
    two = _dev(np.full(h["u"].shape, SENTINEL, dtype), gpu, offset)
    _call(osg, gpu, d, size, halo, zeta=two)
    osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table([two]), 1, osg._lib.ptr_table([nd]), (C.c_int8 * 1)(0),
                                                (C.c_double * 1)(MASK_VALUE), *size, *halo, osg._lib.ft_of(two.dtype),
                                                osg._lib.current_stream_ptr(gpu)))
    _assert_parent(two.cpu().numpy(), got, "two passes")
    # NaN wherever only masked nodes read
    wet = np.arange(1, Nz + 1)[:, None, None] > n[None]                                  # (Nz, Ny, Nx): the nodes that are computed
    need_u, need_v = np.zeros(h["u"].shape, bool), np.zeros(h["u"].shape, bool)
    for dj in (0, -1):
        need_u[Hz:Hz + Nz, Hy + dj:Hy + dj + Ny, Hx:Hx + Nx] |= wet
    for di in (0, -1):
        need_v[Hz:Hz + Nz, Hy:Hy + Ny, Hx + di:Hx + di + Nx] |= wet
    nan = dict(h)
    nan["u"], nan["v"] = np.where(need_u, h["u"], dtype(np.nan)), np.where(need_v, h["v"], dtype(np.nan))
    assert np.isnan(nan["u"][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]).any()
    got = _call(osg, gpu, _device(nan, gpu, offset), size, halo, nd, MASK_VALUE)
    assert not np.isnan(got).any()
    _assert_parent(got, want, "NaN under the mask")


def test_latitude_bands_equal_the_global_field(osg, gpu):
    """40 x 24 x 3, halo 4, filled global parents; three bands of 8 rows cut as rows jstart - Hy .. jend + Hy of the parents and the metrics:
    each band's zeta equals the matching rows of the global zeta (row 1 of a band reads its south halo row, the neighbour's last row)"""
    size, halo, dtype = (40, 24, 3), (4, 4, 4), F64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case((size, halo, dtype))
    glob = h["want"]
    rows = 8
    for b in range(3):
        lo = b * rows                                              # 0-based padded row of the band's row jstart - Hy
        cut = {k: np.ascontiguousarray(h[k][..., lo:lo + rows + 2 * Hy, :]) for k in ("u", "v", "dx_fc", "dy_cf", "az_ff")}
        bsize = (Nx, rows, Nz)
        got = _call(osg, gpu, _device(cut, gpu), bsize, halo)
        _assert_parent(got[Hz:Hz + Nz, Hy:Hy + rows, Hx:Hx + Nx], glob[Hz:Hz + Nz, Hy + lo:Hy + lo + rows, Hx:Hx + Nx], ("band", b))
        _assert_parent(got, _ref(cut, bsize, halo), ("band parent", b))


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
def _grid_fields(osg, gpu, size, halo, tdt, grid=None, seed=3):
    grid = grid or osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
    gen = torch.Generator(device=gpu).manual_seed(seed)
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v])
    return grid, u, v


def _grid_ref(grid, u, v, size, halo, n_ff=None):
    g = getattr(grid, "underlying_grid", grid)
    host = {"u": u.data.cpu().numpy(), "v": v.data.cpu().numpy()}
    for k in ("dx_fc", "dy_cf", "az_ff"):
        host[k] = g.arrays[k].cpu().numpy()
    with np.errstate(all="ignore"):
        z = interior_vorticity(host["u"], host["v"], host["dx_fc"], host["dy_cf"], host["az_ff"], size, halo)
    if n_ff is not None:
        z = np.where(np.arange(1, size[2] + 1)[:, None, None] <= n_ff[None], z.dtype.type(0), z)
    return z


PACKAGE = [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)]


@pytest.mark.parametrize("size,halo,tdt", PACKAGE, ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_vertical_vorticity_on_a_built_grid(osg, gpu, size, halo, tdt):
    """on the grid's own metric arrays: the interior equals the reference; with fill_halos zeta's halos are what fill_halo_regions gives a
    field with that interior, without it they stay as they were"""
    grid, u, v = _grid_fields(osg, gpu, size, halo, tdt)
    want = _grid_ref(grid, u, v, size, halo)
    zeta = osg.vertical_vorticity(u, v)
    assert zeta.loc == (osg.Face, osg.Face, osg.Center) and zeta.grid is grid and osg.is_zipper(zeta.boundary_conditions.north)
    assert zeta.boundary_conditions.north.condition == 1
    _assert_parent(zeta.interior().cpu().numpy(), want, "interior")
    filled = osg.Field((osg.Face, osg.Face, osg.Center), grid)
    filled.interior().copy_(torch.from_numpy(want))
    osg.fill_halo_regions([filled])
    _assert_parent(zeta.data.cpu().numpy(), filled.data.cpu().numpy(), "filled halos")
    out = osg.Field((osg.Face, osg.Face, osg.Center), grid)
    out.data.fill_(SENTINEL)
    assert osg.vertical_vorticity(u, v, out=out, fill_halos=False) is out
    bare = np.full(tuple(out.data.shape), SENTINEL, want.dtype)
    bare[halo[2]:halo[2] + size[2], halo[1]:halo[1] + size[1], halo[0]:halo[0] + size[0]] = want
    _assert_parent(out.data.cpu().numpy(), bare, "halos left alone")


def test_plan_replays_in_a_graph_and_allocates_nothing(osg, gpu):
    size, halo = (48, 40, 6), (4, 4, 4)
    grid, u, v = _grid_fields(osg, gpu, size, halo, torch.float64)
    zeta = osg.Field((osg.Face, osg.Face, osg.Center), grid)
    plan = osg.vorticity_plan(u, v, zeta)
    assert plan() is zeta                                          # eager warm-up (first-call work outside the capture)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    plan()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            plan()
    torch.cuda.current_stream().wait_stream(side)
    gen = torch.Generator(device=gpu).manual_seed(17)
    for _ in range(2):                                             # u changes, the graph is replayed: the results are the eager ones
        u.data.uniform_(-1, 1, generator=gen)
        osg.fill_halo_regions([u])
        zeta.data.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = osg.vertical_vorticity(u, v)
        _assert_parent(zeta.data.cpu().numpy(), eager.data.cpu().numpy(), "replay")
        _assert_parent(zeta.interior().cpu().numpy(), _grid_ref(grid, u, v, size, halo), "replay against the reference")


def test_vertical_vorticity_field_and_compute(osg, gpu):
    size, halo = (20, 12, 3), (3, 2, 1)
    grid, u, v = _grid_fields(osg, gpu, size, halo, torch.float64)
    zeta = osg.VerticalVorticityField(u, v)
    assert zeta.loc == (osg.Face, osg.Face, osg.Center) and not zeta.data.any()          # nothing computed yet
    assert osg.compute_(zeta) is zeta
    _assert_parent(zeta.data.cpu().numpy(), osg.vertical_vorticity(u, v).data.cpu().numpy(), "compute_")
    v.data.mul_(2)                                                 # compute! again after the operands changed
    osg.compute_(zeta)
    _assert_parent(zeta.interior().cpu().numpy(), _grid_ref(grid, u, v, size, halo), "recomputed")


def test_immersed_grid_masks_the_peripheral_nodes_in_the_same_call(osg, gpu):
    size, halo = (48, 40, 6), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo, z=(-1, 0))
    zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
    rng = np.random.default_rng(19)
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)))
    _, u, v = _grid_fields(osg, gpu, size, halo, torch.float64, grid=ibg)
    n = ibg.column_counts["ff"].cpu().numpy()
    assert (n == Nz).any() and (n < Nz).any()
    zeta = osg.vertical_vorticity(u, v)
    _assert_parent(zeta.interior().cpu().numpy(), _grid_ref(ibg, u, v, size, halo, n), "masked interior")
    two = osg.vertical_vorticity(u, v, mask_immersed=False, fill_halos=False)
    _assert_parent(two.interior().cpu().numpy(), _grid_ref(ibg, u, v, size, halo), "unmasked interior")
    osg.mask_immersed_field(two, 0)
    osg.fill_halo_regions([two])
    _assert_parent(two.data.cpu().numpy(), zeta.data.cpu().numpy(), "mask pass + fill")


# ---- past 2^31 elements --------------------------------------------------------------------------------------------------------------------
def test_float32_past_2g_elements(osg, gpu):
    """8640 x 4320 x 64, halo 4, Float32: 2.7e9 elements per parent, so the element offsets of the upper levels need 64 bits.  Data drawn on
    the device; levels k = 1 and k = Nz compared in full with numpy on those two slabs, and zeta's bottom and top halo planes still hold the
    sentinel"""
    size, halo = (8640, 4320, 64), (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = _shapes(size, halo)
    assert parent[0] * parent[1] * parent[2] > 1 << 31
    gen = torch.Generator(device=gpu).manual_seed(5)
    d = {k: torch.empty(parent, dtype=torch.float32, device=gpu).uniform_(-1, 1, generator=gen) for k in ("u", "v")}
    for k in ("dx_fc", "dy_cf", "az_ff"):
        d[k] = torch.empty(plane, dtype=torch.float32, device=gpu).uniform_(0.5, 2, generator=gen)
    d["zeta"] = torch.full(parent, SENTINEL, dtype=torch.float32, device=gpu)
    osg._lib.check_operators(osg._lib.operators_lib().tpg_vertical_vorticity(d["u"].data_ptr(), d["v"].data_ptr(), d["zeta"].data_ptr(), d["dx_fc"].data_ptr(),
                                              d["dy_cf"].data_ptr(), d["az_ff"].data_ptr(), None, 0.0, *size, *halo, osg._lib.TPG_F32,
                                              osg._lib.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    host = {k: d[k].cpu().numpy() for k in ("dx_fc", "dy_cf", "az_ff")}
    for level in (Hz, Hz + Nz - 1):                                # parent planes of k = 1 and k = Nz
        slab = {k: d[k][level:level + 1].cpu().numpy() for k in ("u", "v")}
        want = interior_vorticity(slab["u"], slab["v"], host["dx_fc"], host["dy_cf"], host["az_ff"], (Nx, Ny, 1), (Hx, Hy, 0))
        got = d["zeta"][level].cpu().numpy()
        _assert_parent(got[None, Hy:Hy + Ny, Hx:Hx + Nx], want, ("level", level))
        edge = np.ones(got.shape, bool)
        edge[Hy:Hy + Ny, Hx:Hx + Nx] = False
        assert (got[edge] == SENTINEL).all()
    assert bool((d["zeta"][Hz - 1] == SENTINEL).all()) and bool((d["zeta"][Hz + Nz] == SENTINEL).all())
