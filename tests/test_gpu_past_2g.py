"""GPU tests of the five passes added after the halo-5 work -- tpg_mask_immersed_fields, tpg_fill_open_faces,
tpg_fill_value_gradient_halos, tpg_field_extrema, tpg_cell_advection_timescale -- on parents whose INTERIOR crosses element offset 2^31
(and byte offsets 2^32, 2^33 and, Float64, 2^34), as every field of BASELINE config 5 (8640 x 4320 x 100) does.  An `int` product in one
of their offsets (plane * k + sx * j + e0, crow + c * W) would pass every smaller test and is caught here.

Geometry: the smallest config-5-shaped parents that get there, 8640 x 4320 x 64 --
    halo (4, 4, 4) Float64, plain 16-B chunks: 2 694 855 168 padded elements (20.1 GiB), offset 2^31 in padded plane 57 = interior level 54
    halo (5, 5, 5) Float32, GEN W = 4:         2 771 633 000 padded elements (10.3 GiB), offset 2^31 in padded plane 57 = interior level 53
Three cells are planted or named in every test (three_cells): the first interior cell at or past 2^31, the last interior cell, one below 2^30.

References are built on the device FROM THE DEFINITIONS with operations that are exact -- indexing, comparison, clone, masked_fill_, amin /
amax -- level by level; arithmetic is done on the host in numpy on the one row or plane concerned (value_gradient_ref.extrapolate,
reduction_ref.cell_advection_timescale), except the Float64 timescale, whose torch abs / divide / add / max are IEEE.  Whole parents are
compared with torch.equal on integer views, so that a store that wrapped to a low address shows up as well.  Every test holds its peak of
device memory under half the card."""
import contextlib
import ctypes as C
import gc
import time

import numpy as np
import pytest
import torch

from reduction_ref import cell_advection_timescale, same
from value_gradient_ref import GRADIENT, VALUE, extrapolate

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIZE = (8640, 4320, 64)
CASES = [(SIZE, (4, 4, 4), F64), (SIZE, (5, 5, 5), F32)]
TWO31, TWO30 = 1 << 31, 1 << 30
SOUTH, BOTTOM, TOP = 1, 2, 4
SENTINEL = 12345.0


def _id(case):
    size, halo, dtype = case
    return "h" + "".join(map(str, halo)) + ("-f64" if dtype == F64 else "-f32")


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _budget(gpu, what):
    """wall time and peak device memory of the block, printed; the peak stays under half the card"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu)
    print(f"\n[past-2g] {what}: {time.perf_counter() - t0:.1f} s, peak {peak / 2**30:.1f} GiB")
    assert peak < torch.cuda.get_device_properties(gpu).total_memory / 2, peak


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def shape_of(size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)


def offset_of(cell, size, halo):
    """element offset in the padded parent of the interior cell (k, j, i), 0-based"""
    (k, j, i), (Hx, Hy, Hz) = cell, halo
    _, sy, sx = shape_of(size, halo)
    return ((k + Hz) * sy + (j + Hy)) * sx + (i + Hx)


def interior_cell_at_or_past(offset, size, halo):
    """the interior cell (k, j, i), 0-based, that contains element `offset` of the padded parent -- or, where that element is a halo
    cell, the first interior cell after it"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    _, sy, sx = shape_of(size, halo)
    pk, rem = divmod(offset, sy * sx)
    pj, pi = divmod(rem, sx)
    if pi >= Hx + Nx:                                              # east halo: the next row
        pj, pi = pj + 1, Hx
    pi = max(pi, Hx)
    if pj >= Hy + Ny:                                              # north halo: the next plane
        pk, pj, pi = pk + 1, Hy, Hx
    if pj < Hy:
        pj, pi = Hy, Hx
    if pk < Hz:
        pk, pj, pi = Hz, Hy, Hx
    assert pk < Hz + Nz, "no interior cell at or past this offset"
    cell = (pk - Hz, pj - Hy, pi - Hx)
    assert offset_of(cell, size, halo) >= offset
    return cell


def three_cells(size, halo):
    """the first interior cell at or past 2^31, the last interior cell, one interior cell below 2^30"""
    Nx, Ny, Nz = size
    low = interior_cell_at_or_past(TWO30 - 3 * (Nx + 2 * halo[0]), size, halo)
    cells = [interior_cell_at_or_past(TWO31, size, halo), (Nz - 1, Ny - 1, Nx - 1), low]
    assert offset_of(cells[0], size, halo) >= TWO31 and offset_of(cells[1], size, halo) > TWO31 and offset_of(low, size, halo) < TWO30
    return cells


def _parent(cell, halo):
    return (cell[0] + halo[2], cell[1] + halo[1], cell[2] + halo[0])


def _tdt(dtype):
    return torch.float64 if dtype == F64 else torch.float32


def _ints(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _random(gpu, shape, tdt, seed, lo=-1.0, hi=1.0):
    return torch.empty(shape, dtype=tdt, device=gpu).uniform_(lo, hi, generator=torch.Generator(device=gpu).manual_seed(seed))


def _nan_halos(t, halo):
    """every halo cell of the padded parent (3-D) or padded plane (2-D) NaN, by indexing"""
    h = halo[::-1][-t.ndim:]
    for dim, x in enumerate(h):
        if x:
            t.narrow(dim, 0, x).fill_(float("nan"))
            t.narrow(dim, t.shape[dim] - x, x).fill_(float("nan"))
    return t


def _count_plane(gpu, size, seed, open_columns=()):
    """a count plane random in 0..Nz, columns 0..7 of every row at Nz (the stores reach the top level), 8..15 at 0, `open_columns` at 0"""
    Nx, Ny, Nz = size
    n = torch.randint(0, Nz + 1, (Ny, Nx), dtype=torch.int32, device=gpu, generator=torch.Generator(device=gpu).manual_seed(seed))
    n[:, :8] = Nz
    n[:, 8:16] = 0
    for j, i in open_columns:
        n[j, i] = 0
    return n


def _bound(n, zl, nz_field):
    """masked / left-out levels of a field on count plane n (1-based k <= bound): n for a z-Center field, min(n + 1, nz_field - 1) for a
    z-Face field"""
    return torch.clamp(n + 1, max=nz_field - 1) if zl else n


def test_the_geometry_is_the_one_the_table_states():
    """2 694 855 168 and 2 771 633 000 padded elements; offset 2^31 in padded plane 57, an interior level; the helper inverts offset_of,
    and steps from every kind of halo cell to the next interior cell"""
    for (size, halo, dtype), elems in zip(CASES, (2694855168, 2771633000)):
        shape = shape_of(size, halo)
        assert int(np.prod(shape, dtype=np.int64)) == elems
        assert TWO31 // (shape[1] * shape[2]) == 57 and halo[2] <= 57 < halo[2] + size[2]
        assert elems * np.dtype(dtype).itemsize > (1 << 34 if dtype == F64 else 1 << 33)
        for cell in three_cells(size, halo) + [(0, 0, 0), (5, 17, 0), (5, 17, size[0] - 1)]:
            assert interior_cell_at_or_past(offset_of(cell, size, halo), size, halo) == cell
        assert interior_cell_at_or_past(0, size, halo) == (0, 0, 0)
        assert interior_cell_at_or_past(offset_of((3, 9, size[0] - 1), size, halo) + 1, size, halo) == (3, 10, 0)
        assert interior_cell_at_or_past(offset_of((3, size[1] - 1, size[0] - 1), size, halo) + 1, size, halo) == (4, 0, 0)
        k31 = three_cells(size, halo)[0][0]
        assert k31 == 57 - halo[2]


# ---- tpg_mask_immersed_fields ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mask_writes_every_masked_level_past_2g(osg, gpu, case):
    """one z-Center and one z-Face sentinel field in one table, a random count plane with columns at Nz (the stores reach the top level,
    past 2^31: levels 54.. / 53.. of the interior) and at 0: each parent equals the sentinel with `value` wherever level <= n (z-Face:
    min(n + 1, Nz - 1)), bit for bit on the whole parent -- the cell at 2^31, the last interior cell and a cell below 2^30 among them"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = _tdt(dtype)
    at31, last, low = three_cells(size, halo)
    with _budget(gpu, f"mask {_id(case)}"):
        n = _count_plane(gpu, size, 3)
        n[last[1], last[2]] = Nz                                   # the last interior cell is written (z-Center) / the one below it (z-Face)
        n[at31[1], at31[2]] = Nz
        n[low[1], low[2]] = Nz
        fields = [torch.full(shape_of(size, halo), SENTINEL, dtype=tdt, device=gpu) for _ in range(2)]
        values = (0.25, -2.5)
        lib = osg._lib.lib()
        osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table(fields), 2, osg._lib.ptr_table([n, n]), (C.c_int8 * 2)(0, 1),
                                                    (C.c_double * 2)(*values), *size, *halo, osg._lib.ft_of(tdt), osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        for zl, f, value in zip((0, 1), fields, values):
            bound = _bound(n, zl, Nz)
            want = torch.full(shape_of(size, halo), SENTINEL, dtype=tdt, device=gpu)
            for k in range(Nz):
                want[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(k + 1 <= bound, value)
            assert want[_parent(at31, halo)].item() == value and want[_parent(low, halo)].item() == value
            assert want[_parent(last, halo)].item() == (SENTINEL if zl else value)
            assert torch.equal(_ints(f), _ints(want)), zl
            del want
        del fields


# ---- tpg_fill_open_faces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_open_faces_past_2g(osg, gpu, case):
    """the south face of a (Center, Face, Center) field at every level (rows past 2^31 from level 54 / 53 on) and the bottom and top faces
    of a (Center, Center, Face) field (Nz + 1 levels: the top face plane lies wholly past 2^31 and ends at the last interior cell), once
    with scalar and once with array conditions: the parent equals a clone with those faces assigned by indexing (the rule of open_ref.py)"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = _tdt(dtype)
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    lib = osg._lib.lib()

    def call(f, fsize, sides, values, conds):
        osg._lib.check(lib.tpg_fill_open_faces(osg._lib.ptr_table([f]), 1, (C.c_uint8 * 1)(sides), (C.c_double * 3)(*values),
                                               (C.c_void_p * 3)(*[None if c is None else c.data_ptr() for c in conds]), *fsize, *halo,
                                               osg._lib.ft_of(tdt), osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()

    with _budget(gpu, f"open faces {_id(case)}"):
        # v: south
        v = _random(gpu, shape_of(size, halo), tdt, 1)
        want = v.clone()
        assert offset_of((Nz - 1, 0, 0), size, halo) > TWO31
        call(v, size, SOUTH, (0.25, 0.0, 0.0), (None, None, None))
        want[Hz:Hz + Nz, Hy, :] = 0.25
        assert torch.equal(_ints(v), _ints(want)), "south, scalar"
        cs = _random(gpu, (Nz, sx), tdt, 2)
        call(v, size, SOUTH, (0.0, 0.0, 0.0), (cs, None, None))
        want[Hz:Hz + Nz, Hy, :] = cs
        assert torch.equal(_ints(v), _ints(want)), "south, array"
        del v, want
        # w: bottom and top, Nz + 1 levels
        wsize = (Nx, Ny, Nz + 1)
        w = _random(gpu, shape_of(wsize, halo), tdt, 3)
        want = w.clone()
        assert offset_of((Nz, 0, 0), wsize, halo) > TWO31
        call(w, wsize, BOTTOM | TOP, (0.0, -0.5, 2.0), (None, None, None))
        want[Hz, Hy:Hy + Ny, :] = -0.5
        want[Hz + Nz, Hy:Hy + Ny, :] = 2.0
        assert torch.equal(_ints(w), _ints(want)), "bottom / top, scalar"
        cb, ct = _random(gpu, (sy, sx), tdt, 4), _random(gpu, (sy, sx), tdt, 5)
        call(w, wsize, BOTTOM | TOP, (0.0, 0.0, 0.0), (None, cb, ct))
        want[Hz, Hy:Hy + Ny, :] = cb[Hy:Hy + Ny]
        want[Hz + Nz, Hy:Hy + Ny, :] = ct[Hy:Hy + Ny]
        assert torch.equal(_ints(w), _ints(want)), "bottom / top, array"
        assert want[_parent((Nz, Ny - 1, Nx - 1), halo)].item() == ct[Hy + Ny - 1, Hx + Nx - 1].item()
        del w, want


# ---- tpg_fill_value_gradient_halos ----------------------------------------------------------------------------------------------------------
#            south             bottom              top
VG_ROUNDS = [((VALUE, "array"), (GRADIENT, "scalar"), (VALUE, "array")),
             ((GRADIENT, "scalar"), (VALUE, "array"), (GRADIENT, "scalar")),
             ((VALUE, "scalar"), (GRADIENT, "array"), (GRADIENT, "array")),
             ((GRADIENT, "array"), (VALUE, "scalar"), (VALUE, "scalar"))]


@pytest.mark.parametrize("rnd", range(len(VG_ROUNDS)), ids=lambda r: "round%d" % r)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_value_gradient_halos_past_2g(osg, gpu, case, rnd):
    """the south pass (row 0 of every interior level: the upper levels' rows lie past 2^31) and then the bottom / top pass (plane 0, and
    plane Nz + 1 wholly past 2^31) on one random field; over the four rounds every side sees Value and Gradient with a scalar and with an
    array condition.  Expected: a clone whose row 0 is replaced per interior level and whose planes 0 and Nz + 1 are replaced, the values
    from value_gradient_ref.extrapolate on host copies of the clone's source rows / planes, the condition and the metric"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = _tdt(dtype)
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    lib = osg._lib.lib()
    specs = VG_ROUNDS[rnd]
    dz = (dtype(10.0), dtype(12.5))
    with _budget(gpu, f"value / gradient {_id(case)} round {rnd}"):
        c = _random(gpu, shape_of(size, halo), tdt, 10 + rnd)
        want = c.clone()
        dy = _nan_halos(_random(gpu, (sy, sx), tdt, 20, 3e4, 6e4), (0, Hy, 0))         # rows j <= 0 NaN: row j = 1 is the one that is read
        kinds, values, conds, hosts = [], [], [], []
        for side, (kind, form) in enumerate(specs):
            rows = Nz if side == 0 else sy
            kinds.append(kind)
            if form == "array":
                t = _random(gpu, (rows, sx), tdt, 30 + side)
                conds.append(t)
                values.append(0.0)
                hosts.append(t.cpu().numpy())
            else:
                s = dtype((-0.75, 0.5, 1.5)[side])
                conds.append(None)
                values.append(float(s))
                hosts.append(s)
        table = (osg._lib.ptr_table([c]), 1)
        tail = ((C.c_uint8 * 3)(*kinds), (C.c_double * 3)(*values), (C.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in conds]),
                dy.data_ptr(), float(dz[0]), float(dz[1]), *size, *halo, osg._lib.ft_of(tdt), osg._lib.current_stream_ptr(gpu))
        osg._lib.check(lib.tpg_fill_value_gradient_halos(*table, SOUTH, *tail))
        osg._lib.check(lib.tpg_fill_value_gradient_halos(*table, BOTTOM | TOP, *tail))
        torch.cuda.synchronize()
        assert offset_of((Nz - 1, -1, 0), size, halo) > TWO31 and offset_of((Nz, 0, 0), size, halo) > TWO31
        with np.errstate(all="raise"):
            new = extrapolate(kinds[0], want[Hz:Hz + Nz, Hy].cpu().numpy(), hosts[0], dy[Hy].cpu().numpy()[None, :], False)
            want[Hz:Hz + Nz, Hy - 1] = torch.from_numpy(new).to(gpu)
            new = extrapolate(kinds[1], want[Hz].cpu().numpy(), hosts[1], dz[0], False)       # after the south pass: its row 0 is a source
            want[Hz - 1] = torch.from_numpy(new).to(gpu)
            new = extrapolate(kinds[2], want[Hz + Nz - 1].cpu().numpy(), hosts[2], dz[1], True)
            want[Hz + Nz] = torch.from_numpy(new).to(gpu)
        assert torch.equal(_ints(c), _ints(want))
        del c, want


# ---- tpg_field_extrema ------------------------------------------------------------------------------------------------------------------------
def _extrema(osg, gpu, tensors, size, halo, planes=None, zlocs=None):
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


def _amin_amax(t, size, halo, bound=None):
    """(min, max, max|c|) over the interior of the parent `t` by amin / amax, level by level; with `bound`, the nodes k <= bound (1-based)
    are left out"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    los, his = [], []
    for k in range(Nz):
        x = t[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx]
        if bound is None:
            los.append(x.amin())
            his.append(x.amax())
        else:
            out = k + 1 <= bound
            los.append(x.masked_fill(out, float("inf")).amin())
            his.append(x.masked_fill(out, float("-inf")).amax())
    lo, hi = float(torch.stack(los).amin().item()), float(torch.stack(his).amax().item())
    return lo, hi, max(-lo, hi)


def _assert_triple(got, want, what):
    for g, w, name in zip(got, want, ("min", "max", "maxabs")):
        assert same(g, w), (what, name, float(g), float(w))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_extrema_past_2g(osg, gpu, case):
    """three fields in one call, random interiors, every halo cell NaN: the three values equal amin / amax over the interior views; then
    +5 / -7 planted in turn at the first interior cell at or past 2^31, at the last interior cell and at a cell below 2^30, each found;
    then with count planes, zloc Center and Face (and one field without a plane), the left-out nodes holding NaN: the masked amin / amax"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = _tdt(dtype)
    cells = three_cells(size, halo)
    with _budget(gpu, f"extrema {_id(case)}"):
        fields = [_nan_halos(_random(gpu, shape_of(size, halo), tdt, 40 + f, -1.0 - f, 1.0 + f), halo) for f in range(3)]
        want = [_amin_amax(t, size, halo) for t in fields]
        assert all(w[0] < -0.99 and w[1] > 0.99 for w in want)
        got = _extrema(osg, gpu, fields, size, halo)
        for f in range(3):
            _assert_triple(got[f], want[f], ("plain", f))
        for cell in cells:
            at = _parent(cell, halo)
            keep = fields[1][at].item()
            for planted in (5.0, -7.0):
                fields[1][at] = planted
                got = _extrema(osg, gpu, fields, size, halo)
                lo, hi = (want[1][0], planted) if planted > 0 else (planted, want[1][1])
                _assert_triple(got[1], (lo, hi, max(-lo, hi)), (planted, cell))
                _assert_triple(got[0], want[0], (planted, cell, 0))
                _assert_triple(got[2], want[2], (planted, cell, 2))
            fields[1][at] = keep
        # the NotImmersed condition: the planted cells stay counted (their columns are ocean), the left-out nodes hold NaN
        n = _count_plane(gpu, size, 7, [(j, i) for _, j, i in cells])
        masked = []
        for f, zl in ((0, 0), (1, 1)):
            bound = _bound(n, zl, Nz)
            masked.append(_amin_amax(fields[f], size, halo, bound))
            for k in range(Nz):
                fields[f][Hz + k, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(k + 1 <= bound, float("nan"))
        assert torch.isnan(fields[0][Hz + Nz - 1, Hy + 3, Hx]).item() and not torch.isnan(fields[1][Hz + Nz - 1, Hy + 3, Hx]).item()
        got = _extrema(osg, gpu, fields, size, halo, [n, n, None], [0, 1, 0])
        _assert_triple(got[0], masked[0], "masked, Center")
        _assert_triple(got[1], masked[1], "masked, Face")
        _assert_triple(got[2], want[2], "no plane")
        at = _parent(cells[0], halo)
        fields[0][at] = 9.0                                        # past 2^31, in an ocean column: counted
        got = _extrema(osg, gpu, fields, size, halo, [n, n, None], [0, 1, 0])
        _assert_triple(got[0], (masked[0][0], 9.0, 9.0), "masked, planted")
        assert np.isnan(_extrema(osg, gpu, fields, size, halo)[:2]).all()          # without the planes the NaNs count
        del fields


# ---- tpg_cell_advection_timescale -------------------------------------------------------------------------------------------------------------
def _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo, ncc=None):
    lib = osg._lib.lib()
    out = torch.full((1,), 777.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(lib.tpg_reduce_workspace_bytes(1, *size)) // 8, dtype=torch.float64, device=gpu)
    osg._lib.check(lib.tpg_cell_advection_timescale(u.data_ptr(), v.data_ptr(), w.data_ptr(), dx.data_ptr(), dy.data_ptr(), dz.data_ptr(),
                                                    None if ncc is None else ncc.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                    *size, *halo, osg._lib.ft_of(u.dtype), osg._lib.current_stream_ptr(gpu)))
    return out.item()


def _tau_float64(u, v, w, dx, dy, dz, size, halo, ncc=None):
    """1 / max(|u| / dx + |v| / dy + |w| / dz) in Float64 torch arithmetic (IEEE abs, divide, add, max), left to right, level by level;
    with ncc the cells k <= ncc are left out (s >= 0: a left-out cell counts as 0)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert u.dtype == torch.float64
    inner = (slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    idx, idy = dx[inner], dy[inner]
    tops = []
    for k in range(Nz):
        s = u[Hz + k][inner].abs() / idx + v[Hz + k][inner].abs() / idy + w[Hz + k][inner].abs() / dz[k]
        if ncc is not None:
            s = s.masked_fill(k + 1 <= ncc, 0.0)
        tops.append(s.amax())
    smax = torch.stack(tops).amax().item()
    return np.float64(1.0) / np.float64(smax) if smax != 0 else np.inf


def _metrics(gpu, size, halo, tdt):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    dx = _nan_halos(_random(gpu, (sy, sx), tdt, 50, 3e4, 6e4), halo)
    dy = _nan_halos(_random(gpu, (sy, sx), tdt, 51, 3e4, 6e4), halo)
    dz = torch.linspace(0.5, 2.0, Nz, dtype=torch.float64).to(tdt).to(gpu)          # a stretched z: every face its own spacing
    return dx, dy, dz


def test_timescale_float64_past_2g(osg, gpu):
    """Float64, halo 4: random u, v (64 levels) and w (65), NaN halos, random metrics, a stretched dz -- held bit for bit to the whole-array
    torch reference; a maximum of s planted in turn at the three cells (2^31, last, below 2^30) is found; with n_cc, NaNs inside immersed
    cells past 2^31 change nothing; a NaN at w's level Nz + 1 (the last plane, past 2^31) changes nothing"""
    size, halo, dtype = CASES[0]
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = torch.float64
    wsize = (Nx, Ny, Nz + 1)
    cells = three_cells(size, halo)
    with _budget(gpu, "timescale f64"):
        u = _nan_halos(_random(gpu, shape_of(size, halo), tdt, 60), halo)
        v = _nan_halos(_random(gpu, shape_of(size, halo), tdt, 61), halo)
        w = _nan_halos(_random(gpu, shape_of(wsize, halo), tdt, 62, -1e-3, 1e-3), halo)
        dx, dy, dz = _metrics(gpu, size, halo, tdt)
        want = _tau_float64(u, v, w, dx, dy, dz, size, halo)
        assert np.isfinite(want) and want > 0
        got = _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo)
        assert same(got, want), (got, float(want))
        for cell in cells:
            at = _parent(cell, halo)
            keep = u[at].item()
            u[at] = 1e6
            planted = _tau_float64(u, v, w, dx, dy, dz, size, halo)
            assert planted < want / 100
            got = _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo)
            assert same(got, planted), (cell, got, float(planted))
            u[at] = keep
        top = (Hz + Nz, Hy + Ny - 1, Hx + Nx - 1)                  # w's level Nz + 1, the last interior cell of the parent
        keep = w[top].item()
        w[top] = float("nan")
        assert same(_tau(osg, gpu, u, v, w, dx, dy, dz, size, halo), want)
        w[top] = keep
        ncc = _count_plane(gpu, size, 9)
        masked = _tau_float64(u, v, w, dx, dy, dz, size, halo, ncc)
        k31 = cells[0][0] + 1                                      # the first level that lies wholly past 2^31
        for k in range(k31, Nz):                                   # the immersed cells of those levels hold NaN and huge values
            out = k + 1 <= ncc
            u[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(out, float("nan"))
            w[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(out, 1e300)
        assert offset_of((k31, 0, 0), size, halo) > TWO31 and torch.isnan(u[Hz + Nz - 1, Hy + Ny - 1, Hx]).item()
        got = _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo, ncc)
        assert same(got, masked), (got, float(masked))
        assert np.isnan(_tau(osg, gpu, u, v, w, dx, dy, dz, size, halo))           # without the plane the NaNs count
        del u, v, w


def test_timescale_float32_past_2g(osg, gpu):
    """Float32, halo 5 (GEN).  torch's Float32 division is not ours to assume, so no device arithmetic is the reference: the velocities are
    zero except at one planted cell per run (2^31, last, below 2^30) and tau comes from that cell's operands through
    reduction_ref.cell_advection_timescale on a one-cell host array; then a random background whose s is bounded analytically below half
    the planted s; with n_cc, a NaN inside an immersed cell past 2^31 changes nothing; a NaN at w's level Nz + 1 changes nothing"""
    size, halo, dtype = CASES[1]
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = torch.float32
    wsize = (Nx, Ny, Nz + 1)
    cells = three_cells(size, halo)
    with _budget(gpu, "timescale f32"):
        u = _nan_halos(torch.zeros(shape_of(size, halo), dtype=tdt, device=gpu), halo)
        v = _nan_halos(torch.zeros(shape_of(size, halo), dtype=tdt, device=gpu), halo)
        w = _nan_halos(torch.zeros(shape_of(wsize, halo), dtype=tdt, device=gpu), halo)
        dx, dy, dz = _metrics(gpu, size, halo, tdt)
        assert _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo) == np.inf
        planted = (F32(3.0), F32(-2.5), F32(1.75))

        def expected(cell):
            k, j, i = cell
            one = lambda x: np.array(x, dtype=F32)
            return cell_advection_timescale(one([[[planted[0]]]]), one([[[planted[1]]]]), one([[[planted[2]]], [[0.0]]]),
                                            one([[dx[Hy + j, Hx + i].item()]]), one([[dy[Hy + j, Hx + i].item()]]), one([dz[k].item()]),
                                            (1, 1, 1), (0, 0, 0))

        def plant(cell, values):
            at = _parent(cell, halo)
            for t, x in zip((u, v, w), values):
                t[at] = float(x)

        for cell in cells:
            plant(cell, planted)
            want = expected(cell)
            assert 0 < want < 1 / 0.02                             # s >= 1.75 / 2
            got = _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo)
            assert same(got, want), (cell, got, float(want))
            plant(cell, (0.0, 0.0, 0.0))
        # a random background: |u|, |v|, |w| <= 1e-4, dx, dy >= 3e4, dz >= 0.5, so s <= 2e-4 / 3e4 + 1e-4 / 0.5 (+ rounding) < 2.1e-4,
        # below half of the planted s >= 1.75 / dz[k] >= 0.875: the maximum of s is the planted cell's
        for t, seed in ((u, 70), (v, 71), (w, 72)):
            t.copy_(_random(gpu, t.shape, tdt, seed, -1e-4, 1e-4))
            _nan_halos(t, halo)
        bound = 2e-4 / 3e4 + 1e-4 / 0.5
        assert bound * 1.001 < (1.75 / 2.0) / 2 and float(dz.max()) <= 2.0 and float(dz.min()) >= 0.5
        assert float(dx[Hy:Hy + Ny, Hx:Hx + Nx].amin()) >= 3e4 and float(dy[Hy:Hy + Ny, Hx:Hx + Nx].amin()) >= 3e4
        background = _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo)
        assert background > 1 / (bound * 1.001)
        ncc = _count_plane(gpu, size, 11, [(j, i) for _, j, i in cells])
        ncc[Ny - 1, Nx - 2] = Nz                                   # the column next to the last one is land up to the top level
        for cell in cells:
            plant(cell, planted)
            want = expected(cell)
            got = _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo)
            assert same(got, want), (cell, got, float(want))
            top = (Hz + Nz, Hy + Ny - 1, Hx + Nx - 1)              # w's level Nz + 1
            keep = w[top].item()
            w[top] = float("nan")
            assert same(_tau(osg, gpu, u, v, w, dx, dy, dz, size, halo), want)
            w[top] = keep
            land = (Hz + Nz - 1, Hy + Ny - 1, Hx + Nx - 2)         # an immersed cell past 2^31
            keep = u[land].item()
            u[land] = float("nan")
            assert same(_tau(osg, gpu, u, v, w, dx, dy, dz, size, halo, ncc), want)
            assert np.isnan(_tau(osg, gpu, u, v, w, dx, dy, dz, size, halo))
            u[land] = keep
            plant(cell, (0.0, 0.0, 0.0))
        del u, v, w


# ---- the package surface at the Float64 size ---------------------------------------------------------------------------------------------------
def _bottom(lam, phi):
    """a bottom that is a function of (lambda, phi) only: about half of the cells of z = (-1, 0) immersed, pole boxes and southern cap land"""
    rl, rp = torch.deg2rad(lam), torch.deg2rad(phi)
    h = -(0.5 + 0.5 * torch.sin(3 * rl) * torch.cos(2 * rp) + 0.2 * torch.cos(5 * rl) * torch.sin(4 * rp)).clamp(0, 1)
    land = (((lam - 70).abs() < 5) & ((55 - phi).abs() < 5)) | (((lam - 250).abs() < 5) & ((55 - phi).abs() < 5)) | (phi < -78)
    return torch.where(land, torch.zeros_like(h), h)


def test_package_surface_past_2g(osg, gpu):
    """ImmersedBoundaryGrid(TripolarGrid(size = (8640, 4320, 64)), GridFittedBottom(f(lambda, phi))), Float64, the default halo:
    mask_immersed_field on a CenterField and a ZFaceField, field_extrema of the two and cell_advection_timescale(u, v, w) against the same
    device references, the count plane recomputed from its definition c = #{k : zc[k] <= h}.  The fields' upper levels lie past 2^31"""
    from orthogonalsphericalshellgrids.jl_amd.reductions import z_face_spacings
    size, halo = SIZE, (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    tdt = torch.float64
    with _budget(gpu, "package surface f64"):
        grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
        ibg = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(_bottom))
        h = ibg.immersed_boundary.bottom_height.data[0, Hy:Hy + Ny, Hx:Hx + Nx]
        zc = grid.z_centers[Hz:Hz + Nz]
        n = torch.zeros((Ny, Nx), dtype=torch.int32, device=gpu)
        for k in range(Nz):
            n += (zc[k] <= h).to(torch.int32)
        assert torch.equal(n, ibg.column_counts["cc"])
        frac = float(n.float().mean()) / Nz
        assert 0.3 < frac < 0.8 and bool((n == Nz).any()) and bool((n == 0).any())
        c, w = osg.CenterField(ibg), osg.ZFaceField(ibg)
        for f, seed in ((c, 80), (w, 81)):
            f.data.copy_(_random(gpu, f.data.shape, tdt, seed, 0.5, 1.5))
        for f, zl in ((c, 0), (w, 1)):
            want = f.data.clone()
            bound = _bound(n, zl, f.Nz)
            for k in range(f.Nz):
                want[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(k + 1 <= bound, 0.0)
            osg.mask_immersed_field(f)
            assert torch.equal(_ints(f.data), _ints(want)), f.loc
            del want
        # field_extrema: the masked nodes hold NaN now and are left out
        wants = []
        for f, zl in ((c, 0), (w, 1)):
            fsize = (Nx, Ny, f.Nz)
            bound = _bound(n, zl, f.Nz)
            wants.append(_amin_amax(f.data, fsize, halo, bound))
            for k in range(f.Nz):
                f.data[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(k + 1 <= bound, float("nan"))
        got = osg.field_extrema([c, w])
        _assert_triple(got[0], wants[0], "c")
        _assert_triple(got[1], wants[1], "w")
        assert 0.5 <= wants[0][0] < 0.5001 and 1.4999 < wants[1][1] <= 1.5
        del c
        gc.collect()
        torch.cuda.empty_cache()
        # cell_advection_timescale: u holds NaN in its immersed cells
        u, v = osg.XFaceField(ibg), osg.YFaceField(ibg)
        u.data.copy_(_random(gpu, u.data.shape, tdt, 82))
        v.data.copy_(_random(gpu, v.data.shape, tdt, 83))
        w.data.copy_(_random(gpu, w.data.shape, tdt, 84, -1e-3, 1e-3))
        for k in range(Nz):
            u.data[Hz + k, Hy:Hy + Ny, Hx:Hx + Nx].masked_fill_(k + 1 <= n, float("nan"))
        dz = z_face_spacings(grid).to(gpu)
        want = _tau_float64(u.data, v.data, w.data, grid.arrays["dx_fc"], grid.arrays["dy_cf"], dz, size, halo, n)
        got = osg.cell_advection_timescale(u, v, w)
        assert same(got, want), (got, float(want))
        assert 0 < want < np.inf                                   # the bottom covers the two nodes of row Ny where dx_fc = 0
        del u, v, w
