"""GPU tests of w from continuity and the horizontal divergence: tpg_w_from_continuity through the C ABI, and compute_w_from_continuity /
horizontal_divergence / continuity_plan / HorizontalDivergenceField / compute_ through the package.  Compared BIT FOR BIT with
tests/continuity_ref.py (numpy in the fields' type: every operation of the rule is one correctly rounded IEEE operation, so the reference is
exact and there is no tolerance anywhere in this file); NaNs compare by NaN-ness; no case and no cell is left out of a comparison.

Shapes: the smallest at which each path can go wrong -- the reference's own test size with one level (w has two); the minimum halo (the east /
north read is the halo's only cell); rows off the 16-B grid with an odd Hx (the element-aligned chunks); the model halo 5; Float32 with
Nx = 2 mod 4 (8-B chunks); one shape with more work items than resident threads and Ny a multiple of none of the row counts an item may own;
and one case past 2^31 elements.  dz_c is random in [0.5, 2], so a wrong k index cannot hide."""
import ctypes as C

import numpy as np
import pytest
import torch

from continuity_ref import cells_read, interior_w_and_divergence, same_bits, w_and_divergence
from gpu_harness import _assert_parent, _dev, _free_hbm, _id  # noqa: F401
from immersed_ref import draw_columns, heights_of
from special_values import pool

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#         size            halo       element type
TABLE = [((10, 10, 1), (4, 4, 4), F64),            # the reference's own test size; one level: w has two
         ((20, 12, 3), (1, 1, 1), F64),            # the minimum halo: the east / north read is the halo's only cell
         ((20, 12, 3), (1, 1, 1), F32),
         ((20, 12, 3), (3, 2, 1), F64),            # rows off the 16-B grid, odd Hx: the element-aligned chunks
         ((48, 40, 6), (5, 5, 5), F64),            # the model halo
         ((48, 40, 6), (5, 5, 5), F32),
         ((50, 40, 3), (4, 4, 4), F32),            # Nx = 2 mod 4: 8-B chunks
         ((2304, 1283, 2), (4, 4, 4), F64)]        # >= 321 row tiles x 1152 chunks: more items than are resident; 1283 = 4 * 320 + 3 is odd
SENTINEL = 12345.0
MASK_VALUE = 0.1                                   # not representable: converted once to the field type
FORMS = {"both": (True, True), "w": (True, False), "div": (False, True)}


def _shapes(size, halo):
    """(parent of u, v, div; parent of w; plane)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)


INPUTS = ("u", "v", "dy_fc", "dx_cf", "az_cc", "dz_c")
_CASES = {}


def _ref(h, size, halo, n_cc=None, value=0.0):
    """the reference parents (w, div) from sentinel-filled ones"""
    parent, wparent, _ = _shapes(size, halo)
    T = h["u"].dtype
    with np.errstate(all="ignore"):
        return w_and_divergence(h["u"], h["v"], np.full(wparent, SENTINEL, T), np.full(parent, SENTINEL, T), h["dy_fc"], h["dx_cf"], h["az_cc"],
                                h["dz_c"], size, halo, n_cc, value)


def _case(case):
    """host arrays of a case, random in EVERY cell (halos included), and the reference parents of w and div from sentinel-filled ones:
    computed once per case, shared by the tests, never modified (tests copy what they change)"""
    if case not in _CASES:
        size, halo, dtype = case
        parent, _, plane = _shapes(size, halo)
        rng = np.random.default_rng([*size, *halo, np.dtype(dtype).itemsize])
        h = {"u": rng.uniform(-1, 1, parent).astype(dtype), "v": rng.uniform(-1, 1, parent).astype(dtype),
             "dy_fc": rng.uniform(0.5, 2, plane).astype(dtype), "dx_cf": rng.uniform(0.5, 2, plane).astype(dtype),
             "az_cc": rng.uniform(0.5, 2, plane).astype(dtype), "dz_c": rng.uniform(0.5, 2, size[2]).astype(dtype)}
        h["want_w"], h["want_div"] = _ref(h, size, halo)
        for a in h.values():
            a.setflags(write=False)
        _CASES[case] = h
    return _CASES[case]


def _device(h, gpu, offset=0):
    return {k: _dev(h[k], gpu, offset) for k in INPUTS}


def _call(osg, gpu, d, size, halo, form="both", n_cc=None, value=0.0, offset=0):
    """tpg_w_from_continuity on the device arrays d into fresh sentinel-filled outputs -> the whole parents (w, div) on the host, None for
    an output the form leaves out"""
    lib = osg._lib.continuity_lib()
    parent, wparent, _ = _shapes(size, halo)
    T = {torch.float64: F64, torch.float32: F32}[d["u"].dtype]
    has_w, has_div = FORMS[form]
    w = _dev(np.full(wparent, SENTINEL, T), gpu, offset) if has_w else None
    div = _dev(np.full(parent, SENTINEL, T), gpu, offset) if has_div else None
    ptr = lambda t: None if t is None else t.data_ptr()
    osg._lib.check_continuity(lib.tpg_w_from_continuity(
        d["u"].data_ptr(), d["v"].data_ptr(), ptr(w), ptr(div), d["dy_fc"].data_ptr(), d["dx_cf"].data_ptr(), d["az_cc"].data_ptr(),
        d["dz_c"].data_ptr(), ptr(n_cc), value, *size, *halo, osg._lib.ft_of(d["u"].dtype), osg._lib.current_stream_ptr(gpu)))
    return (None if w is None else w.cpu().numpy()), (None if div is None else div.cpu().numpy())


def _assert_forms(osg, gpu, d, size, halo, want_w, want_div, what, n_cc=None, value=0.0, offset=0):
    """w only, div only and both: each output equals the reference's parent, and the both-form's w equals the w-only form's"""
    ws = {}
    for form, (has_w, has_div) in FORMS.items():
        w, div = _call(osg, gpu, d, size, halo, form, n_cc, value, offset)
        assert (w is not None) == has_w and (div is not None) == has_div
        if has_w:
            _assert_parent(w, want_w, (what, form, "w"))
            ws[form] = w
        if has_div:
            _assert_parent(div, want_div, (what, form, "div"))
    _assert_parent(ws["both"], ws["w"], (what, "w of both forms"))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_interior_is_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, offset):
    """random data in every cell, the outputs' parents pre-filled with a sentinel: the whole parents equal the reference's -- the interior the
    rule, w[., ., 1] = +0, every halo cell and both of w's extra halo planes still the sentinel -- for w only, div only and both, with every
    pointer on the 16-B grid and with every pointer one element past an allocation"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    want_w, want_div = h["want_w"], h["want_div"]
    # the reference parents themselves: sentinel exactly on the halo cells, +0 on face 1
    for want, levels in ((want_w, Nz + 1), (want_div, Nz)):
        halo_cells = np.ones(want.shape, bool)
        halo_cells[Hz:Hz + levels, Hy:Hy + Ny, Hx:Hx + Nx] = False
        assert (want[halo_cells] == SENTINEL).all() and not (want[~halo_cells] == SENTINEL).any()
    face1 = want_w[Hz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert (face1 == 0).all() and not np.signbit(face1).any()
    assert want_w.shape[0] == want_div.shape[0] + 1
    _assert_forms(osg, gpu, _device(h, gpu, offset), size, halo, want_w, want_div, "parent", offset=offset)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_no_cell_outside_the_stencil_is_read(osg, gpu, case, offset):
    """every cell of u, v and the metrics that the rule does not read is NaN: the result has no NaN and equals the clean one"""
    size, halo, dtype = case
    h = _case(case)
    read = cells_read(size, halo)
    poisoned = {k: np.where(read[k], h[k], dtype(np.nan)) for k in read}
    assert all(np.isnan(poisoned[k]).sum() == (~read[k]).sum() for k in read) and all(np.isnan(poisoned[k]).any() for k in read)
    poisoned["dz_c"] = h["dz_c"]
    w, div = _call(osg, gpu, _device(poisoned, gpu, offset), size, halo, offset=offset)
    assert not np.isnan(w).any() and not np.isnan(div).any()
    _assert_parent(w, h["want_w"], "poisoned w")
    _assert_parent(div, h["want_div"], "poisoned div")


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max planted in 5 % of the cells of u and v and 3 % of each metric plane (az_cc = +-0 among them: 1 / 0):
    bit for bit numpy's, which computes the same IEEE operations.  The scan carries a NaN or an Inf upward, so the shares are small enough
    that the top face still holds finite values beside NaN and Inf"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    rng = np.random.default_rng([7, *size, *halo])
    p = pool(dtype)
    planted = {"dz_c": h["dz_c"]}
    for name, share in (("u", 0.05), ("v", 0.05), ("dy_fc", 0.03), ("dx_cf", 0.03), ("az_cc", 0.03)):
        a = h[name].copy()
        where = rng.random(a.shape) < share
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
        planted[name] = a
    # whatever the draw gave the small shapes: a zero area of either sign and a NaN velocity in the interior (1 / +-0; NaN up the column)
    planted["az_cc"][Hy, Hx], planted["az_cc"][Hy + Ny - 1, Hx + Nx - 1] = 0.0, -0.0
    planted["u"][Hz, Hy + 1, Hx + 1] = np.nan
    want_w, want_div = _ref(planted, size, halo)
    top = want_w[Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    # a column's top face is finite if none of the 4 Nz velocity cells and 5 metric cells it reads was planted -- fewer than that are lost,
    # since most of the pool (zeros, subnormals, 1, 1000 ...) poisons nothing
    assert np.isnan(top).any() and np.isinf(top).any() and np.isfinite(top).mean() >= 0.95 ** (4 * Nz) * 0.97 ** 5
    _assert_forms(osg, gpu, _device(planted, gpu, offset), size, halo, want_w, want_div, "special values", offset=offset)


_PLANES = {}


def _count_plane(case):
    """a (Center, Center) count plane for a drawn bottom (land columns, open columns, everything between): c = #{k : zc[k] <= h} of heights
    drawn for the counts of draw_columns, with one column above Nz planted (a count plane of a deeper grid).  Computed once per case."""
    if case in _PLANES:
        return _PLANES[case]
    size, halo, dtype = case
    Nx, Ny, Nz = size
    rng = np.random.default_rng([11, *size, *halo])
    zc = ((np.arange(Nz) + 0.5) / Nz).astype(dtype)
    drawn = draw_columns(rng, Nx, Ny, Nz)
    n = (zc[:, None, None] <= heights_of(drawn, zc, rng)[None]).sum(0).astype(np.int32)
    assert np.array_equal(n, drawn)
    n[Ny - 1, Nx - 1] = Nz + 3
    assert n.shape == (Ny, Nx) and (n == 0).any() and (n >= Nz).any() and (n == Nz).any() and (Nz < 2 or ((n > 0) & (n < Nz)).any())
    n.setflags(write=False)
    _PLANES[case] = n
    return n


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_fused_mask_equals_the_reference_and_the_mask_pass(osg, gpu, case, offset):
    """with a count plane: (1) the reference with the mask, in all three forms; (2) the unmasked call followed by tpg_mask_immersed_fields on
    w (zloc Face, its own Nz + 1 levels) and on div (zloc Center), bit for bit on the whole parents"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    n = _count_plane(case)
    want_w, want_div = _ref(h, size, halo, n, MASK_VALUE)
    assert (want_w[Hz, Hy:Hy + Ny, Hx:Hx + Nx] == dtype(MASK_VALUE)).all()               # the bottom face is peripheral in every column
    assert same_bits(want_w[Hz + Nz], h["want_w"][Hz + Nz]) == 0                         # the top face never is: the scan ran unmasked
    d = _device(h, gpu, offset)
    nd = _dev(n, gpu, offset)
    _assert_forms(osg, gpu, d, size, halo, want_w, want_div, "fused mask", nd, MASK_VALUE, offset)
    # the two-pass form
    lib = osg._lib.lib()
    w, div = (_dev(a, gpu, offset) for a in (h["want_w"], h["want_div"]))                # what the unmasked call leaves (checked above)
    for t, zloc, levels in ((w, osg._lib.TPG_FACE, Nz + 1), (div, osg._lib.TPG_CENTER, Nz)):
        osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table([t]), 1, osg._lib.ptr_table([nd]), (C.c_int8 * 1)(zloc),
                                                    (C.c_double * 1)(MASK_VALUE), Nx, Ny, levels, *halo, osg._lib.ft_of(t.dtype),
                                                    osg._lib.current_stream_ptr(gpu)))
    _assert_parent(w.cpu().numpy(), want_w, "two passes w")
    _assert_parent(div.cpu().numpy(), want_div, "two passes div")


def test_latitude_bands_equal_the_global_field(osg, gpu):
    """40 x 24 x 3, halo 4, global parents; three bands of 8 rows cut as rows jstart - Hy .. jend + Hy of the parents and the metrics: each
    band's w and div equal the matching rows of the global ones (row 8 of a band reads its north halo row, the neighbour's first row)"""
    size, halo, dtype = (40, 24, 3), (4, 4, 4), F64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case((size, halo, dtype))
    rows = 8
    for b in range(3):
        lo = b * rows                                              # 0-based padded row of the band's row jstart - Hy
        cut = {k: np.ascontiguousarray(h[k][..., lo:lo + rows + 2 * Hy, :]) for k in INPUTS[:5]}
        cut["dz_c"] = h["dz_c"]
        bsize = (Nx, rows, Nz)
        w, div = _call(osg, gpu, _device(cut, gpu), bsize, halo)
        _assert_parent(w[Hz:Hz + Nz + 1, Hy:Hy + rows, Hx:Hx + Nx], h["want_w"][Hz:Hz + Nz + 1, Hy + lo:Hy + lo + rows, Hx:Hx + Nx], ("band w", b))
        _assert_parent(div[Hz:Hz + Nz, Hy:Hy + rows, Hx:Hx + Nx], h["want_div"][Hz:Hz + Nz, Hy + lo:Hy + lo + rows, Hx:Hx + Nx], ("band div", b))
        bw, bd = _ref(cut, bsize, halo)
        _assert_parent(w, bw, ("band parent w", b))
        _assert_parent(div, bd, ("band parent div", b))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_discrete_gauss_identity_on_the_device(osg, gpu, dtype):
    """integer u, v, power-of-two metrics and spacings, x-periodic halos, through the C ABI: every intermediate is representable, so at each
    level the sum of V * div over the interior equals the north flux row minus the south flux row exactly, and w[Nz+1] = -sum_k d * div"""
    size, halo = (20, 12, 3), (2, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, _, plane = _shapes(size, halo)
    rng = np.random.default_rng(9)
    h = {k: np.exp2(rng.integers(-3, 4, plane)).astype(dtype) for k in ("dy_fc", "dx_cf", "az_cc")}
    h["dz_c"] = np.exp2(rng.integers(-2, 3, Nz)).astype(dtype)
    h["u"], h["v"] = rng.integers(-9, 10, parent).astype(dtype), rng.integers(-9, 10, parent).astype(dtype)
    for k in ("u", "dy_fc"):                                       # the periodic image: column Nx + 1 is column 1
        h[k][..., Hx + Nx:] = h[k][..., Hx:2 * Hx]
    w, div = _call(osg, gpu, _device(h, gpu), size, halo)
    want_w, want_div = _ref(h, size, halo)
    _assert_parent(w, want_w, "w")
    _assert_parent(div, want_div, "div")
    f = lambda a: a.astype(np.float64)                             # sums of small dyadic rationals: exact in float64
    inner = f(div[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx])
    dz = f(h["dz_c"])
    for k in range(Nz):
        total = (f(h["az_cc"][Hy:Hy + Ny, Hx:Hx + Nx]) * dz[k] * inner[k]).sum()
        flux = lambda row: (f(h["dx_cf"][row, Hx:Hx + Nx]) * dz[k] * f(h["v"][Hz + k, row, Hx:Hx + Nx])).sum()
        assert total == flux(Hy + Ny) - flux(Hy), k
    assert np.array_equal(f(w[Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]), -(dz[:, None, None] * inner).sum(0))


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
def _grid_fields(osg, gpu, size, halo, tdt, grid=None, seed=3):
    grid = grid or osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
    gen = torch.Generator(device=gpu).manual_seed(seed)
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v])
    return grid, u, v


def _grid_ref(osg, grid, u, v, size, halo, n_cc=None):
    """(w, div) on the interior from the host copies of the FILLED u and v, the grid's own metric arrays and z_center_spacings"""
    g = getattr(grid, "underlying_grid", grid)
    host = {"u": u.data.cpu().numpy(), "v": v.data.cpu().numpy()}
    for k in ("dy_fc", "dx_cf", "az_cc"):
        host[k] = g.arrays[k].cpu().numpy()
    dz = osg.z_center_spacings(grid, u.data.dtype).numpy().astype(host["u"].dtype)
    w, div = interior_w_and_divergence(host["u"], host["v"], host["dy_fc"], host["dx_cf"], host["az_cc"], dz, size, halo)
    if n_cc is not None:
        Nz = size[2]
        div = np.where(np.arange(1, Nz + 1)[:, None, None] <= n_cc[None], div.dtype.type(0), div)
        w = np.where(np.arange(1, Nz + 2)[:, None, None] <= np.minimum(n_cc + 1, Nz)[None], w.dtype.type(0), w)
    return w, div


def _bare_parent(want, shape, size, halo, levels):
    bare = np.full(shape, SENTINEL, want.dtype)
    bare[halo[2]:halo[2] + levels, halo[1]:halo[1] + size[1], halo[0]:halo[0] + size[0]] = want
    return bare


PACKAGE = [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)]


@pytest.mark.parametrize("size,halo,tdt", PACKAGE, ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_w_and_divergence_on_a_built_grid(osg, gpu, size, halo, tdt):
    """on the grid's own metric arrays, u[Nx+1] the periodic image and v[Ny+1] the sign-flipped fold: the interior equals the reference; with
    fill_halos the outputs' halos are what fill_halo_regions gives a field with that interior, without it they stay as they were"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v = _grid_fields(osg, gpu, size, halo, tdt)
    want_w, want_div = _grid_ref(osg, grid, u, v, size, halo)
    w = osg.compute_w_from_continuity(u, v)
    div = osg.horizontal_divergence(u, v)
    assert w.loc == (osg.Center, osg.Center, osg.Face) and w.grid is grid and w.Nz == Nz + 1
    assert div.loc == (osg.Center, osg.Center, osg.Center) and div.grid is grid
    _assert_parent(w.interior().cpu().numpy(), want_w, "w interior")
    _assert_parent(div.interior().cpu().numpy(), want_div, "div interior")
    for got, want, make in ((w, want_w, osg.ZFaceField), (div, want_div, osg.CenterField)):
        filled = make(grid)
        filled.interior().copy_(torch.from_numpy(want))
        osg.fill_halo_regions([filled])
        _assert_parent(got.data.cpu().numpy(), filled.data.cpu().numpy(), "filled halos")
    # one plan with both outputs, halos left alone
    w2, div2 = osg.ZFaceField(grid), osg.CenterField(grid)
    w2.data.fill_(SENTINEL)
    div2.data.fill_(SENTINEL)
    plan = osg.continuity_plan(u, v, w2, div2, fill_halos=False)
    assert plan() is plan and plan.w is w2 and plan.div is div2
    _assert_parent(w2.data.cpu().numpy(), _bare_parent(want_w, tuple(w2.data.shape), size, halo, Nz + 1), "w halos left alone")
    _assert_parent(div2.data.cpu().numpy(), _bare_parent(want_div, tuple(div2.data.shape), size, halo, Nz), "div halos left alone")
    w2.data.zero_()                                                # as fresh fields are: w's bottom and top halo planes have no condition to fill them
    div2.data.zero_()
    assert osg.compute_w_from_continuity(u, v, w2) is w2 and osg.horizontal_divergence(u, v, out=div2) is div2
    _assert_parent(w2.data.cpu().numpy(), w.data.cpu().numpy(), "w into a given field")
    _assert_parent(div2.data.cpu().numpy(), div.data.cpu().numpy(), "div into a given field")


def test_plan_replays_in_a_graph_and_allocates_nothing(osg, gpu):
    size, halo = (48, 40, 6), (4, 4, 4)
    grid, u, v = _grid_fields(osg, gpu, size, halo, torch.float64)
    w, div = osg.ZFaceField(grid), osg.CenterField(grid)
    plan = osg.continuity_plan(u, v, w, div)
    assert plan() is plan                                          # eager warm-up (first-call work outside the capture)
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
        w.data.zero_()
        div.data.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_w, want_div = _grid_ref(osg, grid, u, v, size, halo)
        _assert_parent(w.data.cpu().numpy(), osg.compute_w_from_continuity(u, v).data.cpu().numpy(), "replay w")
        _assert_parent(div.data.cpu().numpy(), osg.horizontal_divergence(u, v).data.cpu().numpy(), "replay div")
        _assert_parent(w.interior().cpu().numpy(), want_w, "replay w against the reference")
        _assert_parent(div.interior().cpu().numpy(), want_div, "replay div against the reference")


def test_horizontal_divergence_field_and_compute(osg, gpu):
    size, halo = (20, 12, 3), (3, 2, 1)
    grid, u, v = _grid_fields(osg, gpu, size, halo, torch.float64)
    div = osg.HorizontalDivergenceField(u, v)
    assert div.loc == (osg.Center, osg.Center, osg.Center) and not div.data.any()        # nothing computed yet
    assert osg.compute_(div) is div
    _assert_parent(div.data.cpu().numpy(), osg.horizontal_divergence(u, v).data.cpu().numpy(), "compute_")
    v.data.mul_(2)                                                 # compute! again after the operands changed
    osg.compute_(div)
    _assert_parent(div.interior().cpu().numpy(), _grid_ref(osg, grid, u, v, size, halo)[1], "recomputed")


def test_immersed_grid_masks_the_peripheral_nodes_in_the_same_call(osg, gpu):
    size, halo = (48, 40, 6), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo, z=(-1, 0))
    zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
    rng = np.random.default_rng(19)
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)))
    _, u, v = _grid_fields(osg, gpu, size, halo, torch.float64, grid=ibg)
    n = ibg.column_counts["cc"].cpu().numpy()
    assert (n == Nz).any() and (n == 0).any() and ((n > 0) & (n < Nz)).any()
    w, div = osg.compute_w_from_continuity(u, v), osg.horizontal_divergence(u, v)
    want_w, want_div = _grid_ref(osg, ibg, u, v, size, halo, n)
    _assert_parent(w.interior().cpu().numpy(), want_w, "masked w")
    _assert_parent(div.interior().cpu().numpy(), want_div, "masked div")
    w2 = osg.compute_w_from_continuity(u, v, mask_immersed=False, fill_halos=False)
    div2 = osg.horizontal_divergence(u, v, mask_immersed=False, fill_halos=False)
    raw_w, raw_div = _grid_ref(osg, ibg, u, v, size, halo)
    _assert_parent(w2.interior().cpu().numpy(), raw_w, "unmasked w")
    _assert_parent(div2.interior().cpu().numpy(), raw_div, "unmasked div")
    osg.mask_immersed_field([w2, div2], 0)
    osg.fill_halo_regions([w2, div2])
    _assert_parent(w2.data.cpu().numpy(), w.data.cpu().numpy(), "w: mask pass + fill")
    _assert_parent(div2.data.cpu().numpy(), div.data.cpu().numpy(), "div: mask pass + fill")


# ---- past 2^31 elements --------------------------------------------------------------------------------------------------------------------
def test_float32_past_2g_elements(osg, gpu):
    """8640 x 4320 x 64, halo 4, Float32: 2.7e9 elements per parent, so the element offsets of the upper levels need 64 bits.  u = v = 0
    below the top two levels, drawn on the device above: the scan keeps w = +0 exactly up to face Nz - 1; faces Nz - 1 .. Nz + 1 are compared
    in full with numpy on the two top slabs, face 1 and the faces below are +0, and the halo planes still hold the sentinel"""
    size, halo = (8640, 4320, 64), (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, wparent, plane = _shapes(size, halo)
    assert parent[0] * parent[1] * parent[2] > 1 << 31
    gen = torch.Generator(device=gpu).manual_seed(5)
    d = {k: torch.zeros(parent, dtype=torch.float32, device=gpu) for k in ("u", "v")}
    top = slice(Hz + Nz - 2, Hz + Nz)                              # parent planes of levels Nz - 1 and Nz
    for k in ("u", "v"):
        d[k][top].uniform_(-1, 1, generator=gen)
    for k in ("dy_fc", "dx_cf", "az_cc"):
        d[k] = torch.empty(plane, dtype=torch.float32, device=gpu).uniform_(0.5, 2, generator=gen)
    d["dz_c"] = torch.empty(Nz, dtype=torch.float32, device=gpu).uniform_(0.5, 2, generator=gen)
    w = torch.full(wparent, SENTINEL, dtype=torch.float32, device=gpu)
    osg._lib.check_continuity(osg._lib.continuity_lib().tpg_w_from_continuity(
        d["u"].data_ptr(), d["v"].data_ptr(), w.data_ptr(), None, d["dy_fc"].data_ptr(), d["dx_cf"].data_ptr(), d["az_cc"].data_ptr(),
        d["dz_c"].data_ptr(), None, 0.0, *size, *halo, osg._lib.TPG_F32, osg._lib.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    # faces 1 .. Nz - 1: +0 on the interior, bit for bit
    low = w[Hz:Hz + Nz - 1, Hy:Hy + Ny, Hx:Hx + Nx]
    assert not bool(low.view(torch.int32).any())
    del low
    # faces Nz - 1 .. Nz + 1 against numpy on the two top slabs (a scan from +0 over two levels)
    host = {k: d[k].cpu().numpy() for k in ("dy_fc", "dx_cf", "az_cc")}
    slab = {k: d[k][top].cpu().numpy() for k in ("u", "v")}
    want, _ = interior_w_and_divergence(slab["u"], slab["v"], host["dy_fc"], host["dx_cf"], host["az_cc"], d["dz_c"][Nz - 2:].cpu().numpy(),
                                        (Nx, Ny, 2), (Hx, Hy, 0))
    got = w[Hz + Nz - 2:Hz + Nz + 1].cpu().numpy()
    _assert_parent(got[:, Hy:Hy + Ny, Hx:Hx + Nx], want, "top faces")
    assert np.isfinite(want[2]).all() and (want[2] != 0).mean() > 0.99
    # every halo cell still the sentinel: the rows and columns round every interior face, and both halo slabs
    edge = torch.ones(wparent[1:], dtype=torch.bool, device=gpu)
    edge[Hy:Hy + Ny, Hx:Hx + Nx] = False
    for k in (Hz, Hz + Nz // 2, Hz + Nz - 1, Hz + Nz):
        assert bool((w[k][edge] == SENTINEL).all()), k
    assert bool((w[:Hz] == SENTINEL).all()) and bool((w[Hz + Nz + 1:] == SENTINEL).all())
