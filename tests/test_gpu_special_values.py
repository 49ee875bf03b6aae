"""GPU tests of the IEEE edges through the kernels that do arithmetic in the field's type -- tpg_fill_value_gradient_halos,
tpg_cell_advection_timescale, tpg_field_extrema -- and of the scalar values of the store-only passes tpg_mask_immersed_fields and
tpg_fill_open_faces: subnormal operands and results, overflow to Inf, signed zeros, Inf operands, 0/0 and Inf/Inf.  The expectation is
always the numpy reference (value_gradient_ref, reduction_ref, open_ref; the count-plane rule of reduction_ref), which
tests/test_special_value_refs.py holds to exact rational arithmetic on the same cases (tests/special_values.py).  Raw bits are compared,
signed zeros included; where the reference is NaN the result must be NaN, the payload is free.  A build that flushed Float32 subnormals
or swapped the Float32 division for a fast one fails here.

Shapes: the smallest with a plain and a GEN form of every kernel and room for the 361 value pairs -- 48 x 40 x 8 at halo 4 on the 16-B
grid (plain), 50 x 40 x 8 at halo 5 one element past the allocation (GEN; Float32: Nx = 2 mod 4, 8-B chunks in the interior-chunk kernels)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import special_values as sv
from open_ref import open_faces
from reduction_ref import cell_advection_timescale, excluded_from_plane, field_extrema, same
from value_gradient_ref import GRADIENT, VALUE, extrapolate

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#         size          halo       type offset
CASES = [((48, 40, 8), (4, 4, 4), F32, 0),         # plain
         ((48, 40, 8), (4, 4, 4), F64, 0),         # plain
         ((50, 40, 8), (5, 5, 5), F32, 1),         # GEN, 8-B chunks
         ((50, 40, 8), (5, 5, 5), F64, 1)]         # GEN
SENTINEL = 12345.0
SOUTH, BOTTOM, TOP = 1, 2, 4


def _id(case):
    size, halo, dtype, offset = case
    return "x".join(map(str, size)) + "-h" + "".join(map(str, halo)) + ("-f64" if dtype == F64 else "-f32") + ("-gen" if offset else "-plain")


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _tdt(dtype):
    return torch.float64 if dtype == F64 else torch.float32


def _dev(host, gpu, offset):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    host = np.ascontiguousarray(host)
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(host))
    assert offset == 0 or t.data_ptr() % 16 != 0
    return t


def _assert_bits(got, want, what):
    ok = sv.same_bits_or_both_nan(got, want)
    if not ok.all():
        at = tuple(int(x[0]) for x in np.nonzero(~ok))
        raise AssertionError((what, int((~ok).sum()), "cells differ; first at", at, "got", got[at], sv.bits(got)[at], "want", want[at],
                              sv.bits(want)[at]))


def _nan_halos(a, halo):
    """every halo cell of the padded array (2-D or 3-D) NaN"""
    h = halo[::-1][-a.ndim:]
    inner = tuple(slice(x, a.shape[q] - x) for q, x in enumerate(h))
    keep = a[inner].copy()
    a[...] = np.nan
    a[inner] = keep
    return a


# ---- tpg_fill_value_gradient_halos -----------------------------------------------------------------------------------------------------
def _vg_call(osg, gpu, devs, pss, kinds, values, conds, dy, dz, size, halo):
    n = len(devs)
    lib = osg._lib.lib()
    osg._lib.check(lib.tpg_fill_value_gradient_halos(osg._lib.ptr_table(devs), n, pss, (C.c_uint8 * (3 * n))(*kinds), (C.c_double * (3 * n))(*values),
                                                     (C.c_void_p * (3 * n))(*conds), None if dy is None else dy.data_ptr(), float(dz[0]), float(dz[1]),
                                                     *size, *halo, osg._lib.ft_of(devs[0].dtype), osg._lib.current_stream_ptr(gpu)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", [VALUE, GRADIENT], ids=["value", "gradient"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_value_gradient_array_conditions_on_every_pair(osg, gpu, case, kind):
    """every ordered (source cell, condition) pair of the pool -- subnormal, signed-zero, max, Inf and NaN operands; results that are
    subnormal, overflow to Inf, are 0/0 or Inf - Inf -- tiled over (level, column) of row 1 for the south pass and over the source planes of
    the bottom / top pass, the condition an array, with each of the five spacings (the smallest subnormal: d / 2 rounds to 0): the whole
    parent has the reference's bits; at most 30 % of the written cells are NaN in any case"""
    size, halo, dtype, offset = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    src, cond = sv.pairs(dtype)
    shares = []
    for d in sv.spacings(dtype):
        # south: the source is row 1 of the interior levels
        host = np.full((Nz + 2 * Hz, sy, sx), SENTINEL, dtype=dtype)
        host[Hz:Hz + Nz, Hy] = sv.tiled(src, (Nz, sx))
        hc = sv.tiled(cond, (Nz, sx))
        dy = np.full((sy, sx), np.nan, dtype=dtype)
        dy[Hy] = d                                                 # row j = 1 of dy_cf is the one that is read
        dev, dc, ddy = _dev(host, gpu, offset), _dev(hc, gpu, offset), _dev(dy, gpu, offset)
        _vg_call(osg, gpu, [dev], SOUTH, [kind, 0, 0], [0.0] * 3, [dc.data_ptr(), None, None], ddy, (d, d), size, halo)
        with np.errstate(all="ignore"):
            new = extrapolate(kind, host[Hz:Hz + Nz, Hy], hc, d, False)
        host[Hz:Hz + Nz, Hy - 1] = new
        shares.append(float(np.isnan(new).mean()))
        _assert_bits(dev.cpu().numpy(), host, ("south", float(d)))
        # bottom and top in one call: the sources are planes 1 and Nz, the top's pairs in another order
        host = np.full((Nz + 2 * Hz, sy, sx), SENTINEL, dtype=dtype)
        host[Hz] = sv.tiled(src, (sy, sx))
        host[Hz + Nz - 1] = sv.tiled(src[::-1], (sy, sx))
        hb, ht = sv.tiled(cond, (sy, sx)), sv.tiled(cond[::-1], (sy, sx))
        dev, db, dt = _dev(host, gpu, offset), _dev(hb, gpu, offset), _dev(ht, gpu, offset)
        _vg_call(osg, gpu, [dev], BOTTOM | TOP, [0, kind, kind], [0.0] * 3, [None, db.data_ptr(), dt.data_ptr()], None, (d, d), size, halo)
        with np.errstate(all="ignore"):
            nb, nt = extrapolate(kind, host[Hz], hb, d, False), extrapolate(kind, host[Hz + Nz - 1], ht, d, True)
        host[Hz - 1], host[Hz + Nz] = nb, nt
        shares += [float(np.isnan(nb).mean()), float(np.isnan(nt).mean())]
        _assert_bits(dev.cpu().numpy(), host, ("bottom / top", float(d)))
    print(f"{_id(case)} kind {kind}: NaN share of the reference per case min {min(shares):.3f} max {max(shares):.3f}")
    assert max(shares) <= 0.30, shares


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_value_gradient_scalar_conditions_take_every_pool_value(osg, gpu, case):
    """the scalar-condition path -- a double cast to the field type in the kernel -- with one field per pool value (19 fields: two
    batches), every source cell class in every field, both kinds, all three sides, the five spacings: -0.0, subnormals, max, Inf and NaN
    survive the cast and the arithmetic with the reference's bits"""
    size, halo, dtype, offset = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    p = sv.pool(dtype)
    n = p.size
    values = [float(v) for v in p for _ in range(3)]
    for kind in (VALUE, GRADIENT):
        for d in sv.spacings(dtype):
            base = np.full((Nz + 2 * Hz, sy, sx), SENTINEL, dtype=dtype)
            base[Hz:Hz + Nz, Hy] = sv.tiled(p, (Nz, sx))
            base[Hz] = sv.tiled(p, (sy, sx))                       # row 1 of plane 1 is part of it
            base[Hz + Nz - 1] = sv.tiled(p[::-1], (sy, sx))
            dy = np.full((sy, sx), d, dtype=dtype)
            devs = [_dev(base, gpu, offset) for _ in range(n)]
            ddy = _dev(dy, gpu, offset)
            _vg_call(osg, gpu, devs, SOUTH, [kind, kind, kind] * n, values, [None] * (3 * n), ddy, (d, d), size, halo)
            _vg_call(osg, gpu, devs, BOTTOM | TOP, [kind, kind, kind] * n, values, [None] * (3 * n), ddy, (d, d), size, halo)
            for f in range(n):
                want = base.copy()
                with np.errstate(all="ignore"):
                    want[Hz:Hz + Nz, Hy - 1] = extrapolate(kind, want[Hz:Hz + Nz, Hy], p[f], d, False)
                    want[Hz - 1] = extrapolate(kind, want[Hz], p[f], d, False)         # after the south pass: row 0 of plane 1 is a source
                    want[Hz + Nz] = extrapolate(kind, want[Hz + Nz - 1], p[f], d, True)
                _assert_bits(devs[f].cpu().numpy(), want, (kind, float(d), float(p[f])))
            del devs


# ---- tpg_cell_advection_timescale -------------------------------------------------------------------------------------------------------
def _tau(osg, gpu, u, v, w, dx, dy, dz, size, halo):
    lib = osg._lib.lib()
    out = torch.full((1,), 777.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(lib.tpg_reduce_workspace_bytes(1, *size)) // 8, dtype=torch.float64, device=gpu)
    osg._lib.check(lib.tpg_cell_advection_timescale(u.data_ptr(), v.data_ptr(), w.data_ptr(), dx.data_ptr(), dy.data_ptr(), dz.data_ptr(), None,
                                                    out.data_ptr(), ws.data_ptr(), ws.numel() * 8, *size, *halo, osg._lib.ft_of(u.dtype),
                                                    osg._lib.current_stream_ptr(gpu)))
    return out.item()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_timescale_rows_of_special_operands(osg, gpu, case):
    """one launch per row of special_values.timescale_rows, the operands planted at the last interior cell, every other velocity 0, every
    halo cell NaN: a subnormal |u| / 1 (Float32: tau overflows to +Inf for the smallest, is 8.5e37 and FINITE for the largest -- a flushed
    subnormal would give +Inf), max / smallest normal (s = Inf, tau = 0), 0 / 0 and Inf / Inf (NaN), -0.0 velocities (+Inf), a sum that
    overflows (tau = 0), 1 / smallest subnormal; the same through w and dz[k]"""
    size, halo, dtype, offset = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    at = (Nz - 1, Ny - 1, Nx - 1)
    seen = {}
    for name, cell in sv.timescale_rows(dtype):
        u, v, w, dx, dy, dz = sv.timescale_arrays(cell, size, halo, at)
        for a in (u, v, w, dx, dy):
            _nan_halos(a, halo)
        want = cell_advection_timescale(u, v, w, dx, dy, dz, size, halo)
        got = _tau(osg, gpu, *(_dev(a, gpu, offset) for a in (u, v, w, dx, dy, dz)), size, halo)
        print(f"{_id(case)} {name}: tau {got!r} reference {float(want)!r}")
        assert same(got, want), (name, got, float(want))
        seen[name] = got
    if dtype == F32:
        assert seen["smallest subnormal over 1"] == np.inf and 8.4e37 < seen["largest subnormal over 1"] < 8.6e37


# ---- tpg_field_extrema -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_extrema_of_subnormal_zero_max_and_infinite_interiors(osg, gpu, case):
    """five fields in one call, every halo cell NaN: an interior of +-subnormals only (the extrema are subnormal, not 0), of +-0 only, of
    +-max among ordinary values, of ordinary values with +Inf and -Inf present, and with +Inf alone: min, max and max|c| equal the
    numpy reference, as values of the field type widened exactly to double"""
    size, halo, dtype, offset = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng([*size, *halo, offset])
    fi = np.finfo(dtype)
    lsub = np.nextafter(fi.tiny, dtype(0))
    shape = (Nz, Ny, Nx)
    subs = rng.choice(np.array([fi.smallest_subnormal, -fi.smallest_subnormal, dtype(0.3) * fi.tiny, -(dtype(0.3) * fi.tiny)], dtype=dtype), shape)
    subs[Nz - 1, Ny - 1, Nx - 1], subs[0, 0, 0] = lsub, -lsub
    zeros = rng.choice(np.array([0.0, -0.0], dtype=dtype), shape)
    ordinary = lambda: rng.uniform(-1, 1, shape).astype(dtype)
    maxes, infs, pinf = ordinary(), ordinary(), ordinary()
    maxes[Nz - 1, 3, Nx - 1], maxes[1, Ny - 1, 0] = fi.max, -fi.max
    infs[Nz - 1, Ny - 1, 1], infs[0, 2, Nx - 2] = np.inf, -np.inf
    pinf[Nz // 2, Ny // 2, Nx // 2] = np.inf
    inners = [subs, zeros, maxes, infs, pinf]
    hosts = [_nan_halos(np.pad(x, [(h, h) for h in halo[::-1]]), halo) for x in inners]
    devs = [_dev(h, gpu, offset) for h in hosts]
    lib, n = osg._lib.lib(), len(devs)
    out = torch.full((3 * n,), 777.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(lib.tpg_reduce_workspace_bytes(n, *size)) // 8, dtype=torch.float64, device=gpu)
    osg._lib.check(lib.tpg_field_extrema(osg._lib.ptr_table(devs), n, None, None, out.data_ptr(), ws.data_ptr(), ws.numel() * 8, *size, *halo,
                                         osg._lib.ft_of(devs[0].dtype), osg._lib.current_stream_ptr(gpu)))
    got = out.cpu().numpy().reshape(n, 3)
    for f, name in enumerate(("subnormals", "zeros", "max", "both Inf", "+Inf")):
        want = field_extrema(hosts[f], size, halo)
        print(f"{_id(case)} {name}: {got[f].tolist()} reference {[float(x) for x in want]}")
        for g, w, which in zip(got[f], want, ("min", "max", "maxabs")):
            assert same(g, w), (name, which, float(g), float(w))
    assert got[0][0] == -float(lsub) and got[0][1] == float(lsub) and got[0][2] == float(lsub) and float(lsub) != 0
    assert tuple(got[2]) == (-float(fi.max), float(fi.max), float(fi.max)) and tuple(got[3]) == (-np.inf, np.inf, np.inf)


# ---- the scalar values of the store-only passes ------------------------------------------------------------------------------------------------
def _scalars(dtype):
    fi = np.finfo(dtype)
    return np.array([-0.0, fi.smallest_subnormal, fi.max, np.inf, np.nan], dtype=dtype)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mask_writes_the_cast_value_bit_for_bit(osg, gpu, case):
    """tpg_mask_immersed_fields with value = -0.0, the smallest subnormal, max, Inf and NaN (one field each, z-Center and z-Face): the
    masked cells hold (T)value -- the sign of zero kept, the subnormal not flushed, NaN a NaN -- and every other cell its sentinel"""
    size, halo, dtype, offset = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(17)
    vals = _scalars(dtype)
    n = vals.size
    plane = rng.integers(0, Nz + 1, (Ny, Nx)).astype(np.int32)
    plane[:, :8], plane[:, 8:16] = Nz, 0
    dplane = _dev(plane, gpu, offset)
    lib = osg._lib.lib()
    for zl in (0, 1):
        fsize = (Nx, Ny, Nz + zl)
        host = np.full((Nz + zl + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), SENTINEL, dtype=dtype)
        devs = [_dev(host, gpu, offset) for _ in range(n)]
        osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table(devs), n, osg._lib.ptr_table([dplane] * n), (C.c_int8 * n)(*[zl] * n),
                                                    (C.c_double * n)(*[float(v) for v in vals]), *fsize, *halo, osg._lib.ft_of(devs[0].dtype),
                                                    osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        ex = excluded_from_plane(plane, zl, Nz + zl)
        assert 0 < ex.sum() < ex.size
        for f in range(n):
            want = host.copy()
            want[Hz:Hz + Nz + zl, Hy:Hy + Ny, Hx:Hx + Nx][ex] = vals[f]
            _assert_bits(devs[f].cpu().numpy(), want, (zl, float(vals[f])))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_open_faces_write_the_cast_value_bit_for_bit(osg, gpu, case):
    """tpg_fill_open_faces with scalar conditions -0.0, the smallest subnormal, max, Inf and NaN: the south face of a (Center, Face, Center)
    field at every level and the bottom and top faces of a (Center, Center, Face) field hold (T)value bit for bit (NaN: a NaN), every other
    cell its sentinel"""
    size, halo, dtype, offset = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    vals = _scalars(dtype)
    n = vals.size
    lib = osg._lib.lib()
    for fsize, sides in (((Nx, Ny, Nz), SOUTH), ((Nx, Ny, Nz + 1), BOTTOM | TOP)):
        host = np.full((fsize[2] + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), SENTINEL, dtype=dtype)
        devs = [_dev(host, gpu, offset) for _ in range(n)]
        # the top value of field f is the value of field f + 1: bottom and top differ within a field
        table = [(vals[f], vals[f], vals[(f + 1) % n]) for f in range(n)]
        osg._lib.check(lib.tpg_fill_open_faces(osg._lib.ptr_table(devs), n, (C.c_uint8 * n)(*[sides] * n),
                                               (C.c_double * (3 * n))(*[float(x) for t in table for x in t]), (C.c_void_p * (3 * n))(), *fsize, *halo,
                                               osg._lib.ft_of(devs[0].dtype), osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        for f, (s, b, t) in enumerate(table):
            want = open_faces(host.copy(), fsize, halo, s if sides & SOUTH else None, b if sides & BOTTOM else None, t if sides & TOP else None)
            assert (sv.bits(want) != sv.bits(host)).any()
            _assert_bits(devs[f].cpu().numpy(), want, (sides, float(s), float(t)))
