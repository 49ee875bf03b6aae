"""GPU tests of the device reductions: tpg_field_extrema and tpg_cell_advection_timescale through the C ABI, and field_extrema / minimum /
maximum / extrema_plan / cell_advection_timescale / advection_timescale_plan / minimum_xspacing / grid_summary through the package.
Compared BIT FOR BIT with tests/reduction_ref.py (numpy), NaN-ness included; zeros compare by == (the sign of a zero extremum is not
specified).  Min and max are exact and independent of order, so there is no error budget anywhere in this file.

Shapes: the smallest at which each code path can go wrong -- the reference's own test size; rows off the 16-B grid with an odd Hx; halo 5;
Float32 with Nx = 2 mod 4 (8-B chunks); one with more interior rows than blocks (many blocks, many partials, the grid-stride loop)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from immersed_ref import column_counts, draw_columns, heights_of, inactive_cells
from reduction_ref import cell_advection_timescale, excluded_from_plane, excluded_nodes, field_extrema, interior, same

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#         size            halo       element type
TABLE = [((10, 10, 1), (4, 4, 4), F64),            # the reference's own test size
         ((20, 12, 3), (3, 2, 1), F64),            # rows off the 16-B grid, odd Hx
         ((48, 40, 6), (5, 5, 5), F64),            # halo 5
         ((50, 40, 3), (4, 4, 4), F32),            # Nx = 2 mod 4: 8-B chunks
         ((1440, 720, 8), (4, 4, 4), F64)]         # 5760 interior rows: more rows than blocks, 2048 partials per field
SMALL = TABLE[:4]
BOTH = TABLE + [(s, h, F32 if t == F64 else F64) for s, h, t in SMALL]
BLOCKS = 2048                                      # the kernels' block bound: one partial per block


def _id(case):
    size, halo, dtype = case
    return "x".join(map(str, size)) + "-h" + "".join(map(str, halo)) + ("-f64" if dtype == F64 else "-f32")


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _tdt(dtype):
    return torch.float64 if dtype == F64 else torch.float32


def _huge(dtype):
    return dtype(1e300) if dtype == F64 else dtype(1e30)


def _dev(host, gpu, offset=0):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    host = np.ascontiguousarray(host)
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(host))
    assert offset == 0 or t.data_ptr() % 16 != 0
    return t


def _poisoned(inner, halo, poison):
    """the padded parent (or 2-D array) around `inner` with every halo cell poisoned: NaN, or +-huge alternating"""
    pad = [(h, h) for h in halo[::-1][-inner.ndim:]]
    out = np.pad(inner, pad, constant_values=0)
    mask = np.pad(np.zeros(inner.shape, dtype=bool), pad, constant_values=True)
    if poison == "nan":
        out[mask] = np.nan
    else:
        sign = np.where(np.arange(mask.sum()) % 2 == 0, 1, -1).astype(inner.dtype)
        out[mask] = _huge(inner.dtype.type) * sign
    return out


def _extrema(osg, gpu, tensors, size, halo, planes=None, zlocs=None):
    """tpg_field_extrema on device tensors of one geometry -> (n, 3) float64"""
    lib = osg._lib.lib()
    n = len(tensors)
    out = torch.full((3 * n,), 777.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(lib.tpg_reduce_workspace_bytes(n, *size)) // 8, dtype=torch.float64, device=gpu)
    counts = zl = None
    if planes is not None:
        counts = (C.c_void_p * n)(*[None if p is None else p.data_ptr() for p in planes])
        zl = (C.c_int8 * n)(*zlocs)
    osg._lib.check(lib.tpg_field_extrema(osg._lib.ptr_table(tensors), n, counts, zl, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                         *size, *halo, osg._lib.ft_of(tensors[0].dtype), osg._lib.current_stream_ptr(gpu)))
    return out.cpu().numpy().reshape(n, 3)


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("min", "max", "maxabs")):
        assert same(g, w), (what, name, float(g), float(w))


def _random_inner(rng, size, dtype):
    Nx, Ny, Nz = size
    return ((rng.random((Nz, Ny, Nx), dtype=np.float32) - 0.5) * 2).astype(dtype)


# ---- tpg_field_extrema ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", BOTH, ids=_id)
def test_extrema_are_bit_exact_and_no_halo_cell_counts(osg, gpu, case, offset):
    """1, 4 and 17 fields (the last: two batches) of random interiors, every halo cell NaN in one run and +-huge in another: the three
    values of every field equal the reference's over the interior, whatever the halos hold"""
    size, halo, dtype = case
    rng = np.random.default_rng([*size, *halo, offset])
    counts = (1, 4) if size[0] > 1000 else (1, 4, 17)
    inners = [_random_inner(rng, size, dtype) * dtype(1 + f) for f in range(max(counts))]
    want = [field_extrema(np.pad(x, [(h, h) for h in halo[::-1]]), size, halo) for x in inners]
    assert all(w[0] < 0 < w[1] for w in want)
    for poison in ("nan", "huge"):
        devs = [_dev(_poisoned(x, halo, poison), gpu, offset) for x in inners]
        for n in counts:
            got = _extrema(osg, gpu, devs[:n], size, halo)
            for f in range(n):
                _assert_same(got[f], want[f], (poison, n, f))
        del devs


@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_an_extremum_planted_at_every_corner_is_found(osg, gpu, case):
    """the extremum planted in turn at each of the eight interior corners, at the last element of the last block's range and at the last
    element of the first row of the second pass of the grid-stride loop: each is found, as maximum and as minimum"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(5)
    host = _poisoned(_random_inner(rng, size, dtype), halo, "nan")
    dev = _dev(host, gpu)
    rows = Ny * Nz
    nb = min(rows, BLOCKS)                                         # block b owns the rows r = b, b + nb, ...
    last_of_last_block = max(r for r in range(rows - nb, rows) if r % nb == nb - 1)
    spots = {(k, j, i) for k in (0, Nz - 1) for j in (0, Ny - 1) for i in (0, Nx - 1)}
    spots |= {(r // Ny, r % Ny, Nx - 1) for r in (last_of_last_block, min(nb, rows - 1))}
    for k, j, i in sorted(spots):
        at = (Hz + k, Hy + j, Hx + i)
        keep = host[at]
        for planted in (5.0, -7.0):
            host[at] = planted
            dev[at] = planted
            got = _extrema(osg, gpu, [dev], size, halo)[0]
            _assert_same(got, field_extrema(host, size, halo), (planted, k, j, i))
            assert got[1 if planted > 0 else 0] == planted and got[2] == abs(planted)
        host[at] = keep
        dev[at] = float(keep)


@pytest.mark.parametrize("case", SMALL + TABLE[4:], ids=_id)
def test_one_nan_makes_its_field_nan_and_leaves_the_batch_alone(osg, gpu, case):
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(9)
    inners = [_random_inner(rng, size, dtype) for _ in range(4)]
    want = [field_extrema(np.pad(x, [(h, h) for h in halo[::-1]]), size, halo) for x in inners]
    devs = [_dev(_poisoned(x, halo, "huge"), gpu) for x in inners]
    for at in ((Hz + Nz - 1, Hy + Ny - 1, Hx + Nx - 1), (Hz, Hy, Hx),
               (Hz + int(rng.integers(Nz)), Hy + int(rng.integers(Ny)), Hx + int(rng.integers(Nx)))):
        keep = devs[2][at].item()
        devs[2][at] = float("nan")
        got = _extrema(osg, gpu, devs, size, halo)
        assert np.isnan(got[2]).all(), (at, got[2])
        for f in (0, 1, 3):
            _assert_same(got[f], want[f], (at, f))
        devs[2][at] = keep
    for f, g in enumerate(_extrema(osg, gpu, devs, size, halo)):
        _assert_same(g, want[f], ("restored", f))


def test_padded_2d_arrays_reduce_with_nz_1_hz_0(osg, gpu):
    """how the grid reductions reach the call: a (Ny + 2 Hy, Nx + 2 Hx) array as Nz = 1, Hz = 0"""
    for (Nx, Ny), (Hx, Hy), dtype in (((60, 30), (4, 4), F64), ((50, 40), (5, 5), F32), ((20, 12), (3, 2), F64)):
        rng = np.random.default_rng(Nx)
        inner = rng.uniform(1, 2, (Ny, Nx)).astype(dtype)
        host = _poisoned(inner, (Hx, Hy), "nan")
        got = _extrema(osg, gpu, [_dev(host[None], gpu)], (Nx, Ny, 1), (Hx, Hy, 0))[0]
        _assert_same(got, (inner.min(), inner.max(), np.abs(inner).max()), (Nx, Ny))


# ---- the NotImmersed condition -----------------------------------------------------------------------------------------------------------
def _immersed_setup(osg, oracle, gpu, size, halo, dtype, rng):
    """a hand-made bottom (immersed_ref.draw_columns), its filled padded height on the host, the predicate's inactive cells and the four
    count planes on the device (tpg_immersed_column_counts)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    zc = ((np.arange(Nz) + 0.5) / Nz).astype(dtype)
    hin = heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)
    hp = np.zeros((1, Ny + 2 * Hy, Nx + 2 * Hx), dtype=dtype)
    hp[0, Hy:Hy + Ny, Hx:Hx + Nx] = hin
    oracle.fill_halo_regions(hp, 0, 0, 1, (Nx, Ny, 1), (Hx, Hy, 0))
    hp = hp[0]
    planes = {key: torch.empty((Ny, Nx), dtype=torch.int32, device=gpu) for key in ("cc", "fc", "cf", "ff")}
    dh, dz = _dev(hp, gpu), _dev(zc, gpu)
    osg._lib.check(osg._lib.lib().tpg_immersed_column_counts(dh.data_ptr(), dz.data_ptr(), 1, *(planes[k].data_ptr() for k in ("cc", "fc", "cf", "ff")),
                                                             Nx, Ny, Nz, Hx, Hy, osg._lib.ft_of(_tdt(dtype)), osg._lib.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    want = column_counts(hp, zc, size, halo, True)
    for key in planes:
        assert np.array_equal(planes[key].cpu().numpy(), want[key]), key
    return inactive_cells(hp, zc, size, halo, True), planes


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", [TABLE[2], TABLE[3], ((20, 12, 3), (3, 2, 1), F64), ((48, 40, 6), (5, 5, 5), F32)], ids=_id)
def test_not_immersed_leaves_out_exactly_what_the_mask_writes(osg, oracle, gpu, case, offset):
    """the eight locations (z-Face fields have Nz + 1 levels, the top one counted); the left-out nodes hold NaN and huge values and the
    result equals the reference's over the rest, the set taken from the predicate; the same set is what tpg_mask_immersed_fields writes
    into a sentinel field through the same planes; a batch may mix fields with and without a plane; an all-immersed field is empty"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng([*size, *halo, offset, 7])
    ina, planes = _immersed_setup(osg, oracle, gpu, size, halo, dtype, rng)
    lib = osg._lib.lib()
    for zl in (0, 1):
        fsize = (Nx, Ny, Nz + zl)
        locs = [(xl, yl, zl) for xl in (0, 1) for yl in (0, 1)]
        hosts, wants, excl = [], [], []
        for q, loc in enumerate(locs):
            inner = _random_inner(rng, fsize, dtype)
            ex = excluded_nodes(ina, loc, size)
            assert 0 < ex.sum() < ex.size and not (zl and ex[Nz].any())
            inner[Nz + zl - 1, 1, 10 + q] = 3 + q                  # the maximum sits in the top level of an ocean column: counted
            assert not ex[Nz + zl - 1, 1, 10 + q]
            clean = np.pad(inner, [(h, h) for h in halo[::-1]])
            wants.append(field_extrema(clean, fsize, halo, ex))
            assert wants[-1][1] == 3 + q
            inner[ex] = np.where(rng.random(int(ex.sum())) < 0.5, np.nan, _huge(dtype)).astype(dtype)
            hosts.append(_poisoned(inner, halo, "nan"))
            excl.append(ex)
        devs = [_dev(h, gpu, offset) for h in hosts]
        keys = ["cf"[xl] + "cf"[yl] for xl, yl, _ in locs]
        got = _extrema(osg, gpu, devs, fsize, halo, [planes[k] for k in keys], [zl] * 4)
        for q in range(4):
            _assert_same(got[q], wants[q], (zl, locs[q]))
        # the count planes describe the same set, and the mask pass writes exactly it
        sentinels = [_dev(np.full(hosts[0].shape, 12345.0, dtype=dtype), gpu, offset) for _ in locs]
        osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table(sentinels), 4, osg._lib.ptr_table([planes[k] for k in keys]),
                                                    (C.c_int8 * 4)(*[zl] * 4), (C.c_double * 4)(), *fsize, *halo, osg._lib.ft_of(_tdt(dtype)),
                                                    osg._lib.current_stream_ptr(gpu)))
        for q, (s, key) in enumerate(zip(sentinels, keys)):
            written = interior(s.cpu().numpy(), fsize, halo) == 0
            assert np.array_equal(written, excl[q]), (zl, locs[q])
            assert np.array_equal(written, excluded_from_plane(planes[key].cpu().numpy(), zl, Nz + zl))
        # a batch that mixes fields with and without a plane: the one without counts every interior cell (here: NaN)
        mixed = _extrema(osg, gpu, devs[:2], fsize, halo, [planes[keys[0]], None], [zl, zl])
        _assert_same(mixed[0], wants[0], "mixed")
        assert np.isnan(mixed[1]).all()
        if zl == 0:                                                # all-immersed: no cell is counted
            full = torch.full((Ny, Nx), Nz, dtype=torch.int32, device=gpu)
            empty = _extrema(osg, gpu, devs[:1], fsize, halo, [full], [0])[0]
            assert empty[0] == np.inf and empty[1] == -np.inf and empty[2] == -np.inf


# ---- tpg_cell_advection_timescale -----------------------------------------------------------------------------------------------------
def _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo, ncc=None):
    lib = osg._lib.lib()
    out = torch.full((1,), 777.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(lib.tpg_reduce_workspace_bytes(1, *size)) // 8, dtype=torch.float64, device=gpu)
    osg._lib.check(lib.tpg_cell_advection_timescale(u.data_ptr(), v.data_ptr(), w.data_ptr(), dx.data_ptr(), dy.data_ptr(), dz.data_ptr(),
                                                    None if ncc is None else ncc.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                    *size, *halo, osg._lib.ft_of(u.dtype), osg._lib.current_stream_ptr(gpu)))
    return out.item()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", BOTH, ids=_id)
def test_timescale_is_bit_exact(osg, gpu, case, offset):
    """random velocities, random positive metrics, a stretched z; every halo cell of the five arrays NaN in one run and +-huge in another;
    then the special values: all-zero velocities give +Inf, a NaN in w at level Nz gives NaN, a NaN in w at its level Nz + 1 does not;
    with n_cc, huge velocities and NaNs inside immersed cells change nothing"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    wsize = (Nx, Ny, Nz + 1)
    rng = np.random.default_rng([*size, *halo, offset, 11])
    ui, vi, wi = _random_inner(rng, size, dtype), _random_inner(rng, size, dtype), _random_inner(rng, wsize, dtype) * dtype(1e-3)
    dxi, dyi = rng.uniform(3e4, 6e4, (Ny, Nx)).astype(dtype), rng.uniform(3e4, 6e4, (Ny, Nx)).astype(dtype)
    dz = np.cumsum(rng.uniform(0.5, 2, Nz)).astype(dtype)          # a stretched z: every face its own spacing
    ddz = _dev(dz, gpu, offset)
    results = []
    for poison in ("nan", "huge"):
        hu, hv, hw = (_poisoned(x, halo, poison) for x in (ui, vi, wi))
        hdx, hdy = _poisoned(dxi, halo[:2], poison), _poisoned(dyi, halo[:2], poison)
        want = cell_advection_timescale(hu, hv, hw, hdx, hdy, dz, size, halo)
        assert np.isfinite(want) and want > 0
        u, v, w, dx, dy = (_dev(x, gpu, offset) for x in (hu, hv, hw, hdx, hdy))
        got = _tau(osg, gpu, u, v, w, dx, dy, ddz, size, halo)
        assert same(got, want), (poison, got, float(want))
        results.append(got)
    assert results[0] == results[1]
    zero_u, zero_v, zero_w = torch.zeros_like(u), torch.zeros_like(v), torch.zeros_like(w)
    assert _tau(osg, gpu, zero_u, zero_v, zero_w, dx, dy, ddz, size, halo) == np.inf
    top = (Hz + Nz, Hy + Ny // 2, Hx + Nx // 2)                    # w's level Nz + 1
    keep = w[top].item()
    w[top] = float("nan")
    assert _tau(osg, gpu, u, v, w, dx, dy, ddz, size, halo) == results[1]
    w[top] = keep
    last = (Hz + Nz - 1, Hy + Ny - 1, Hx + Nx - 1)                 # w's level Nz, the last cell of the last row
    keep = w[last].item()
    w[last] = float("nan")
    assert np.isnan(_tau(osg, gpu, u, v, w, dx, dy, ddz, size, halo))
    w[last] = keep
    # n_cc: immersed cells hold huge velocities and NaNs
    ncc = rng.integers(0, Nz + 1, (Ny, Nx)).astype(np.int32)
    ncc[:, :2] = Nz
    ncc[:, 2:4] = 0
    ex = excluded_from_plane(ncc, 0, Nz)
    want = cell_advection_timescale(hu, hv, hw, hdx, hdy, dz, size, halo, ncc)
    for arr, junk in ((hu, _huge(dtype)), (hv, np.nan), (hw, -_huge(dtype))):
        interior(arr, (Nx, Ny, arr.shape[0] - 2 * Hz), halo)[:Nz][ex] = junk
    assert same(cell_advection_timescale(hu, hv, hw, hdx, hdy, dz, size, halo, ncc), want)
    u, v, w = (_dev(x, gpu, offset) for x in (hu, hv, hw))
    dn = _dev(ncc, gpu, offset)
    got = _tau(osg, gpu, u, v, w, dx, dy, ddz, size, halo, dn)
    assert same(got, want), (got, float(want))
    assert _tau(osg, gpu, u, v, w, dx, dy, ddz, size, halo, torch.full((Ny, Nx), Nz, dtype=torch.int32, device=gpu)) == np.inf


# ---- the package surface -------------------------------------------------------------------------------------------------------------------
def _loc(osg, loc):
    return tuple(osg.Face if b else osg.Center for b in loc)


def _ref_of_field(f, planes, zl_plane=None):
    host = f.data.cpu().numpy()
    size, halo = (f.Nx, f.Ny, f.Nz), (f.Hx, f.Hy, f.Hz)
    ex = None
    if planes is not None:
        key = ("f" if f.loc[0].__name__ == "Face" else "c") + ("f" if f.loc[1].__name__ == "Face" else "c")
        ex = excluded_from_plane(planes[key].cpu().numpy(), 1 if f.loc[2].__name__ == "Face" else 0, f.Nz)
    return field_extrema(host, size, halo, ex)


@pytest.mark.parametrize("tdt,h", [(torch.float64, 5), (torch.float32, 4)], ids=["f64-halo5", "f32-halo4"])
def test_package_surface_on_a_bare_and_an_immersed_grid(osg, gpu, tdt, h):
    """field_extrema / minimum / maximum, cell_advection_timescale and the plan forms against the numpy reference on the package's own
    arrays (metrics from the grid, dz from z_face_spacings, stretched z); repeated plan calls allocate nothing; a replayed
    torch.cuda.graph gives the eager bits after the fields are changed between replays"""
    size, halo = (48, 40, 6), (h, h, h)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    npt = F64 if tdt == torch.float64 else F32
    faces = [-10.0, -6.0, -3.5, -1.7, -0.9, -0.3, 0.0]
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=faces)
    rng = np.random.default_rng(21)
    zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
    cols = draw_columns(rng, Nx, Ny, Nz)
    cols[Ny - 1, :] = Nz                                           # row Ny is land: the bottom masks the grid's poles, where dx_fc = 0
    ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(heights_of(cols, zc, rng)))
    gen = torch.Generator(device=gpu).manual_seed(3)
    dz = osg.z_face_spacings(grid).numpy().astype(npt)
    assert dz[0] == osg.grids.boundary_z_spacings(grid)[0] and len(set(dz.tolist())) == Nz
    for g, planes in ((grid, None), (ibg, ibg.column_counts)):
        u, v, w, c = osg.XFaceField(g), osg.YFaceField(g), osg.ZFaceField(g), osg.CenterField(g)
        for f in (u, v, w, c):
            f.data.uniform_(-1, 1, generator=gen)                  # halos too: they must not count
        got = osg.field_extrema([u, v, w, c])
        for f, t in zip((u, v, w, c), got):
            assert all(isinstance(x, float) for x in t)
            _assert_same(t, _ref_of_field(f, planes), f.loc)
        assert osg.minimum(u) == got[0][0] and osg.maximum(u) == got[0][1] and osg.maximum(u, abs=True) == got[0][2]
        if planes is not None:                                     # without the condition: the bare grid's answer
            _assert_same(osg.field_extrema([c], not_immersed=False)[0], _ref_of_field(c, None), "not_immersed=False")
        hdx, hdy = grid.arrays["dx_fc"].cpu().numpy(), grid.arrays["dy_cf"].cpu().numpy()
        ncc = None if planes is None else planes["cc"].cpu().numpy()
        want = cell_advection_timescale(u.data.cpu().numpy(), v.data.cpu().numpy(), w.data.cpu().numpy(), hdx, hdy, dz, size, halo, ncc)
        tau = osg.cell_advection_timescale(u, v, w)
        assert isinstance(tau, float) and same(tau, want), (tau, float(want))
        # the bare grid keeps the two nodes of row Ny that sit on the grid's poles, where dx_fc = 0: tau = 0 there; the bottom masks them
        assert tau == 0.0 if planes is None else (0 < tau < np.inf)
        # the plan forms
        eplan, tplan = osg.extrema_plan([u, v, w, c]), osg.advection_timescale_plan(u, v, w)
        eplan(); tplan()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for _ in range(5):
            eplan(); tplan()
        assert torch.cuda.memory_allocated() == before
        assert eplan.result() == got and tplan.result() == tau
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
            eplan(); tplan()
        torch.cuda.current_stream().wait_stream(side)
        for scale in (3.0, 0.25):
            for f in (u, v, w, c):
                f.data.mul_(scale)
            interior_c = osg.interior(c)
            interior_c[Nz - 1, 3, Nx - 1] = 100.0 * scale          # the last element of a row of the top level
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            replayed, rtau = eplan.result(), tplan.result()
            eager, etau = osg.field_extrema([u, v, w, c]), osg.cell_advection_timescale(u, v, w)
            assert replayed == eager and (rtau == etau or (np.isnan(rtau) and np.isnan(etau)))
            for f, t in zip((u, v, w, c), eager):
                _assert_same(t, _ref_of_field(f, planes), (scale, f.loc))
        if planes is None:
            assert eager[3][1] == 25.0
    # z-windowed fields: accepted without the condition, refused with it (as mask_immersed_field refuses them)
    win = osg.Field(_loc(osg, (0, 0, 0)), ibg, indices=(slice(None), slice(None), range(2, 5)))
    win.data.uniform_(-1, 1, generator=gen)
    _assert_same(osg.field_extrema([win], not_immersed=False)[0], _ref_of_field(win, None), "window")
    with pytest.raises(NotImplementedError, match="z-windowed"):
        osg.field_extrema([win])
    bare_win = osg.Field(_loc(osg, (0, 0, 0)), grid, indices=(slice(None), slice(None), range(2, 5)))
    assert osg.field_extrema([bare_win])[0] == (0.0, 0.0, 0.0)
    with pytest.raises(TypeError, match="v must be a Field at"):
        osg.cell_advection_timescale(u, u, w)


def test_readme_transcript_through_the_product(osg, kats, gpu):
    """grid_summary(TripolarGrid(size = (60, 30, 1))) rounded to 6 significant digits (phi: 4 decimals) equals the reference's README
    transcript; minimum_xspacing / minimum_yspacing equal numpy.min of the interior of the matching array at all four locations"""
    k = kats["readme_60x30"]
    grid = osg.TripolarGrid(osg.GPU(0), size=tuple(k["size"]))
    s = osg.grid_summary(grid)
    sig = lambda x: float(f"{x:.6g}")
    assert s["center"][0] == k["center_lambda_phi"][0] and round(s["center"][1], 4) == k["center_lambda_phi"][1]
    assert sig(s["longitude_extent"]) == k["longitude_extent_deg"] and sig(s["latitude_extent"]) == k["latitude_extent_deg"]
    assert sig(s["min_dlambda"]) == k["min_dlambda"] and sig(s["max_dlambda"]) == k["max_dlambda"]
    assert sig(s["min_dphi"]) == k["min_dphi"] and sig(s["max_dphi"]) == k["max_dphi"]
    text = osg.summary(grid)
    lines = text.split("\n")
    assert len(lines) == 5 and lines[0] == repr(grid)
    assert "centered at (λ, φ) = (70.0, 1.8005)" in lines[1]
    assert "extent 359.885 degrees" in lines[2] and "min(Δλ)=0.279019, max(Δλ)=6.32049" in lines[2]
    assert "extent 175.667 degrees" in lines[3] and "min(Δφ)=0.429975, max(Δφ)=5.86207" in lines[3]
    assert "z ∈ [0.0, 1.0]" in lines[4] and "Δz=1.0" in lines[4]
    for tdt, halo in ((torch.float64, (4, 4, 4)), (torch.float32, (5, 5, 5))):
        g = osg.TripolarGrid(osg.GPU(0), tdt, size=(50, 40, 2), halo=halo)
        for LX in (osg.Center, osg.Face):
            for LY in (osg.Center, osg.Face):
                sfx = ("f" if LX is osg.Face else "c") + ("f" if LY is osg.Face else "c")
                assert osg.minimum_xspacing(g, LX, LY) == float(g.interior("dx_" + sfx).cpu().numpy().min()), sfx
                assert osg.minimum_yspacing(g, LX, LY) == float(g.interior("dy_" + sfx).cpu().numpy().min()), sfx
    assert osg.minimum_xspacing(grid) == float(grid.interior("dx_cc").cpu().numpy().min())
