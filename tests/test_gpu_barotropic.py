"""GPU tests of the barotropic mode and the split-explicit velocity correction: tpg_barotropic_mode / tpg_barotropic_correction through the
C ABI, and compute_barotropic_mode / barotropic_correction / the two plans through the package.  Compared BIT FOR BIT with
tests/barotropic_ref.py (numpy in the fields' type: every operation of the rules is one correctly rounded IEEE operation and the column sum
has one order, so the reference is exact and there is no tolerance anywhere in this file); NaNs compare by NaN-ness; no case and no cell is
left out of a comparison.

Shapes (size, halo, Hy2, type): the smallest at which each path can go wrong -- the reference's own test size with one level (the sum is one
product); no halo at all; rows off the 16-B grid with an odd Hx and Hy2 < Hy; the reference's 12-substep extended halo; the model halo 5 with
config 5's Hy2 = 31; Float32 with Nx = 2 mod 4 (8-B chunks); one shape with more work items than are resident; and one case past 2^31
elements.  dz_c is random in [0.5, 2] and depth_of_count random positive, so a wrong k or n index cannot hide."""
import ctypes as C

import numpy as np
import pytest
import torch

import barotropic_ref as ref
from barotropic_ref import same_bits
from continuity_ref import interior_w_and_divergence
from gpu_harness import _dev, _free_hbm  # noqa: F401
from immersed_ref import draw_columns, heights_of
from special_values import pool

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#         size            halo      Hy2  element type
TABLE = [((10, 10, 1), (4, 4, 4), 4, F64),         # the reference's own test size; one level: the sum is one product
         ((20, 12, 3), (0, 0, 0), 0, F64),         # no halo at all
         ((20, 12, 3), (0, 0, 0), 0, F32),
         ((20, 12, 3), (3, 2, 1), 1, F64),         # odd Hx, rows off the 16-B grid, Hy2 < Hy
         ((64, 40, 3), (4, 4, 4), 13, F64),        # the reference's 12-substep extended halo
         ((48, 40, 6), (5, 5, 5), 31, F64),        # the model halo with config 5's Hy2
         ((48, 40, 6), (5, 5, 5), 31, F32),
         ((50, 40, 3), (4, 4, 4), 4, F32),         # Nx = 2 mod 4: 8-B chunks
         ((2304, 1283, 2), (4, 4, 4), 4, F64)]     # 1283 x 1152 chunks: more items than are resident
SENTINEL = 12345.0
MASK_VALUE = 0.1                                   # not representable: converted once to the field type
FORMS = {"both": (True, True), "u": (True, False), "v": (False, True)}
FIELDS = ("u", "v")
PLANES = ("U", "V", "Ubar", "Vbar")


def _id(case):
    size, halo, Hy2, dtype = case
    return "x".join(map(str, size)) + "-h" + "".join(map(str, halo)) + f"-{Hy2}" + ("-f64" if dtype == F64 else "-f32")


def _shapes(size, halo, Hy2):
    """(parent of u, v; 2-D plane)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy2, Nx + 2 * Hx)


_CASES = {}


def _ref_mode(h, size, halo, Hy2, form="both"):
    """the reference planes (Ubar, Vbar) from sentinel-filled ones"""
    _, plane = _shapes(size, halo, Hy2)
    T = h["dz_c"].dtype
    has = FORMS[form]
    return ref.barotropic_mode(h["u"] if has[0] else None, h["v"] if has[1] else None, np.full(plane, SENTINEL, T) if has[0] else None,
                               np.full(plane, SENTINEL, T) if has[1] else None, h["dz_c"], size, halo, Hy2)


def _ref_corr(h, size, halo, Hy2, n_fc=None, n_cf=None, value=0.0, form="both"):
    has = FORMS[form]
    pick = lambda k, q: h[k] if has[q] else None
    return ref.barotropic_correction(pick("u", 0), pick("v", 1), pick("U", 0), pick("V", 1), pick("Ubar", 0), pick("Vbar", 1), h["depth"], size,
                                     halo, Hy2, n_fc if has[0] else None, n_cf if has[1] else None, value)


def _case(case):
    """host arrays of a case, random in EVERY cell (halos included): u, v, the four 2-D planes the correction reads (Ubar, Vbar random like
    U, V: the correction takes them as given), dz_c, depth_of_count; and the references -- the mode's planes from sentinel-filled ones, the
    correction's parents.  Computed once per case, shared by the tests, never modified (tests copy what they change)"""
    if case not in _CASES:
        size, halo, Hy2, dtype = case
        parent, plane = _shapes(size, halo, Hy2)
        rng = np.random.default_rng([*size, *halo, Hy2, np.dtype(dtype).itemsize])
        h = {k: rng.uniform(-1, 1, parent).astype(dtype) for k in FIELDS}
        h.update({k: rng.uniform(-1, 1, plane).astype(dtype) for k in PLANES})
        h["dz_c"] = rng.uniform(0.5, 2, size[2]).astype(dtype)
        h["depth"] = rng.uniform(0.5, 2, size[2] + 1).astype(dtype)
        h["want_Ubar"], h["want_Vbar"] = _ref_mode(h, size, halo, Hy2)
        h["want_u"], h["want_v"] = _ref_corr(h, size, halo, Hy2)
        for a in h.values():
            a.setflags(write=False)
        _CASES[case] = h
    return _CASES[case]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _mode(osg, gpu, h, size, halo, Hy2, form="both", offset=0):
    """tpg_barotropic_mode on device copies of h into fresh sentinel-filled planes -> the whole planes (Ubar, Vbar) on the host, None for a
    pair the form leaves out"""
    _, plane = _shapes(size, halo, Hy2)
    T = h["dz_c"].dtype
    has = FORMS[form]
    src = [_dev(h[k], gpu, offset) if has[q] else None for q, k in enumerate(FIELDS)]
    dst = [_dev(np.full(plane, SENTINEL, T), gpu, offset) if has[q] else None for q in range(2)]
    dz = _dev(h["dz_c"], gpu, offset)
    osg._lib.check_barotropic(osg._lib.barotropic_lib().tpg_barotropic_mode(
        _ptr(src[0]), _ptr(src[1]), _ptr(dst[0]), _ptr(dst[1]), dz.data_ptr(), *size, *halo, Hy2, osg._lib.ft_of(dz.dtype),
        osg._lib.current_stream_ptr(gpu)))
    return tuple(None if t is None else t.cpu().numpy() for t in dst)


def _corr(osg, gpu, h, size, halo, Hy2, form="both", n_fc=None, n_cf=None, value=0.0, offset=0, keep=False):
    """tpg_barotropic_correction in place on fresh device copies of h -> the whole parents (u, v) on the host (`keep`: the device tensors and
    the count planes instead), None for a triple the form leaves out"""
    has = FORMS[form]
    d = {k: _dev(h[k], gpu, offset) if has[q % 2] else None for q, k in enumerate(FIELDS + PLANES)}
    depth = _dev(h["depth"], gpu, offset)
    n = [None if p is None or not has[q] else _dev(p, gpu, offset) for q, p in enumerate((n_fc, n_cf))]
    osg._lib.check_barotropic(osg._lib.barotropic_lib().tpg_barotropic_correction(
        _ptr(d["u"]), _ptr(d["v"]), _ptr(d["U"]), _ptr(d["V"]), _ptr(d["Ubar"]), _ptr(d["Vbar"]), depth.data_ptr(), _ptr(n[0]), _ptr(n[1]), value,
        *size, *halo, Hy2, osg._lib.ft_of(depth.dtype), osg._lib.current_stream_ptr(gpu)))
    if keep:
        return d["u"], d["v"], n
    return tuple(None if d[k] is None else d[k].cpu().numpy() for k in FIELDS)


def _assert_same(got, want, what):
    bad = same_bits(got, want)
    assert bad == 0, (what, bad, "cells differ of", got.size)


def _assert_forms(call, want, what):
    """both fields, u only and v only: every output equals the reference's"""
    for form, has in FORMS.items():
        got = call(form)
        for q in range(2):
            assert (got[q] is not None) == has[q]
            if has[q]:
                _assert_same(got[q], want[q], (what, form, FIELDS[q]))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_whole_parents_are_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, offset):
    """random data in every cell.  The mode: the planes pre-filled with a sentinel equal the reference's -- the interior the rule, every halo
    cell still the sentinel.  The correction: the parents equal the reference's -- the interior the rule, every halo cell its random value.
    For both fields, u only and v only, with every pointer on the 16-B grid and with every pointer one element past an allocation"""
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    for want in (h["want_Ubar"], h["want_Vbar"]):                  # the reference planes themselves: sentinel exactly on the halo cells
        edge = np.ones(want.shape, bool)
        edge[Hy2:Hy2 + Ny, Hx:Hx + Nx] = False
        assert (want[edge] == SENTINEL).all() and not (want[~edge] == SENTINEL).any()
    for k in FIELDS:                                               # the reference parents: the halo cells are the inputs'
        inner = np.zeros(h[k].shape, bool)
        inner[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = True
        assert same_bits(h["want_" + k][~inner], h[k][~inner]) == 0 and (h["want_" + k][inner] != h[k][inner]).mean() > 0.9
    _assert_forms(lambda form: _mode(osg, gpu, h, size, halo, Hy2, form, offset), (h["want_Ubar"], h["want_Vbar"]), "mode")
    _assert_forms(lambda form: _corr(osg, gpu, h, size, halo, Hy2, form, offset=offset), (h["want_u"], h["want_v"]), "correction")


_COUNTS = {}


def _count_planes(case):
    """(n_fc, n_cf): count planes for two drawn bottoms (land columns, open columns, everything between), each with one column above Nz
    planted (a count plane of a deeper grid).  Computed once per case."""
    if case in _COUNTS:
        return _COUNTS[case]
    size, halo, Hy2, dtype = case
    Nx, Ny, Nz = size
    rng = np.random.default_rng([11, *size, *halo])
    zc = ((np.arange(Nz) + 0.5) / Nz).astype(dtype)
    out = []
    for q in range(2):
        drawn = draw_columns(rng, Nx, Ny, Nz)
        n = (zc[:, None, None] <= heights_of(drawn, zc, rng)[None]).sum(0).astype(np.int32)
        assert np.array_equal(n, drawn)
        n[Ny - 1, Nx - 1 - q] = Nz + 3
        assert n.shape == (Ny, Nx) and (n == 0).any() and (n >= Nz).any() and (n == Nz).any() and (Nz < 2 or ((n > 0) & (n < Nz)).any())
        n.setflags(write=False)
        out.append(n)
    _COUNTS[case] = tuple(out)
    return _COUNTS[case]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_no_cell_outside_the_rule_is_read(osg, gpu, case, offset):
    """every cell the rules do not read is NaN -- all halos of u, v, all halos of the 2-D planes, the entries of depth_of_count no count
    selects: the results have no NaN beyond the reference's and equal the clean ones"""
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    n_fc, n_cf = _count_planes(case)
    read = ref.cells_read(size, halo, Hy2, n_fc, n_cf)
    poisoned = {k: np.where(read["field"], h[k], dtype(np.nan)) for k in FIELDS}
    poisoned.update({k: np.where(read["plane"], h[k], dtype(np.nan)) for k in PLANES})
    poisoned["depth"] = np.where(read["depth_of_count"], h["depth"], dtype(np.nan))
    poisoned["dz_c"] = h["dz_c"]
    assert all(np.isnan(poisoned[k]).sum() == (~read["field"]).sum() for k in FIELDS)
    assert all(np.isnan(poisoned[k]).sum() == (~read["plane"]).sum() for k in PLANES)
    assert np.isnan(poisoned["depth"]).sum() == (~read["depth_of_count"]).sum()
    assert max(halo) == 0 or all(np.isnan(poisoned[k]).any() for k in FIELDS + PLANES)
    got = _mode(osg, gpu, poisoned, size, halo, Hy2, offset=offset)
    for q, k in enumerate(("want_Ubar", "want_Vbar")):
        assert not np.isnan(got[q]).any()
        _assert_same(got[q], h[k], ("poisoned mode", k))
    clean = _ref_corr(h, size, halo, Hy2, n_fc, n_cf, MASK_VALUE)
    want = _ref_corr(poisoned, size, halo, Hy2, n_fc, n_cf, MASK_VALUE)
    got = _corr(osg, gpu, poisoned, size, halo, Hy2, "both", n_fc, n_cf, MASK_VALUE, offset)
    for q in range(2):
        assert not np.isnan(clean[q]).any()
        inner = got[q][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert not np.isnan(inner).any()
        _assert_same(inner, clean[q][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], ("poisoned correction interior", q))
        _assert_same(got[q], want[q], ("poisoned correction parent", q))           # the halo cells: the NaNs they held


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max planted in 2 % of the cells of u, v and of the 2-D planes, one NaN and one +Inf explicitly in the
    interior, depth_of_count = +-0 for one count each: bit for bit numpy's, which computes the same IEEE operations"""
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    rng = np.random.default_rng([7, *size, *halo])
    p = pool(dtype)
    planted = {"dz_c": h["dz_c"]}
    for name in FIELDS + PLANES:
        a = h[name].copy()
        where = rng.random(a.shape) < 0.02
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
        planted[name] = a
    planted["u"][Hz, Hy + 1, Hx + 1], planted["u"][Hz + Nz - 1, Hy + 2, Hx + 2] = np.nan, np.inf
    planted["v"][Hz, Hy + 3, Hx + 1], planted["v"][Hz + Nz - 1, Hy + 4, Hx + 2] = np.nan, np.inf
    depth = h["depth"].copy()
    depth[Nz] = 0.0                                                # a land column's depth
    if Nz > 1:
        depth[1] = -0.0
    planted["depth"] = depth
    want = _ref_mode(planted, size, halo, Hy2)
    # a condition on the reference alone: most columns stay finite (a column is lost only to one of its Nz cells drawing a non-finite or
    # overflowing pool value), and NaN and Inf both occur
    ubar = want[0][Hy2:Hy2 + Ny, Hx:Hx + Nx]
    assert np.isfinite(ubar).mean() >= 0.5 and np.isnan(ubar).any() and np.isinf(ubar).any()
    _assert_forms(lambda form: _mode(osg, gpu, planted, size, halo, Hy2, form, offset), want, "special values: mode")
    want = _ref_corr(planted, size, halo, Hy2)
    inner = want[0][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert np.isfinite(inner).mean() >= 0.5 and np.isnan(inner).any() and np.isinf(inner).any()
    _assert_forms(lambda form: _corr(osg, gpu, planted, size, halo, Hy2, form, offset=offset), want, "special values: correction")
    # with count planes every entry of depth_of_count is in use, the two zeros among them
    n_fc, n_cf = _count_planes(case)
    want = _ref_corr(planted, size, halo, Hy2, n_fc, n_cf, MASK_VALUE)
    got = _corr(osg, gpu, planted, size, halo, Hy2, "both", n_fc, n_cf, MASK_VALUE, offset)
    for q in range(2):
        _assert_same(got[q], want[q], ("special values: masked correction", q))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_fused_mask_equals_the_reference_and_the_mask_pass(osg, gpu, case, offset):
    """with count planes: (1) the reference with the mask, in all three forms, and with one plane only; (2) a wholly immersed column --
    depth +0 and U = Ubar there, 0 / 0 -- holds the mask value on every level and no NaN; (3) the unmasked call followed by
    tpg_mask_immersed_fields on u (plane fc, zloc Center) and v (plane cf), bit for bit on the whole parents.  A call without a plane takes
    H = depth_of_count[0] in every column, so (3) runs on a table whose entries are all equal: there the two forms differ in the
    substitution alone, which is what (3) holds to the mask pass"""
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    n_fc, n_cf = _count_planes(case)
    h = dict(_case(case))
    h["depth"] = h["depth"].copy()
    h["depth"][Nz] = 0.0
    land = [np.pad(n >= Nz, ((Hy2, Hy2), (Hx, Hx))) for n in (n_fc, n_cf)]
    h["U"], h["V"] = np.where(land[0], h["Ubar"], h["U"]), np.where(land[1], h["Vbar"], h["V"])
    want = _ref_corr(h, size, halo, Hy2, n_fc, n_cf, MASK_VALUE)
    for q, n in enumerate((n_fc, n_cf)):
        column = np.broadcast_to((n >= Nz)[None], (Nz, Ny, Nx))
        with np.errstate(all="ignore"):
            c = (h[PLANES[q]] - h[PLANES[q + 2]]) / h["depth"][Nz]
        assert np.isnan(c[land[q]]).all() and column.any()          # without the mask: 0 / 0 on every level of a land column
        assert (want[q][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx][column] == dtype(MASK_VALUE)).all() and not np.isnan(want[q]).any()
    _assert_forms(lambda form: _corr(osg, gpu, h, size, halo, Hy2, form, n_fc, n_cf, MASK_VALUE, offset), want, "fused mask")
    one = _ref_corr(h, size, halo, Hy2, None, n_cf, MASK_VALUE)                          # u without a plane: depth_of_count[0], no mask
    got = _corr(osg, gpu, h, size, halo, Hy2, "both", None, n_cf, MASK_VALUE, offset)
    for q in range(2):
        _assert_same(got[q], one[q], ("one plane", q))
    # the two-pass form
    h["depth"] = np.full(Nz + 1, h["depth"][0], dtype)
    raw, want = _ref_corr(h, size, halo, Hy2), _ref_corr(h, size, halo, Hy2, n_fc, n_cf, MASK_VALUE)
    got = _corr(osg, gpu, h, size, halo, Hy2, "both", n_fc, n_cf, MASK_VALUE, offset)
    for q in range(2):
        _assert_same(got[q], want[q], ("fused, one depth", q))
    u, v, _ = _corr(osg, gpu, h, size, halo, Hy2, offset=offset, keep=True)
    for q in range(2):
        _assert_same((u, v)[q].cpu().numpy(), raw[q], ("unmasked", q))
    lib = osg._lib.lib()
    for t, n in ((u, n_fc), (v, n_cf)):
        nd = _dev(n, gpu, offset)
        osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table([t]), 1, osg._lib.ptr_table([nd]), (C.c_int8 * 1)(osg._lib.TPG_CENTER),
                                                    (C.c_double * 1)(MASK_VALUE), *size, *halo, osg._lib.ft_of(t.dtype),
                                                    osg._lib.current_stream_ptr(gpu)))
    _assert_same(u.cpu().numpy(), want[0], "two passes u")
    _assert_same(v.cpu().numpy(), want[1], "two passes v")


def test_latitude_bands_equal_the_global_field(osg, gpu):
    """40 x 24 x 3, halo 4, Hy2 = 6, global parents; three bands of 8 rows cut as rows jstart - Hy .. jend + Hy of the parents (Hy2 for the
    planes) and the matching rows of the count planes: each band's outputs equal the matching rows of the global ones"""
    case = ((40, 24, 3), (4, 4, 4), 6, F64)
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    n_fc, n_cf = _count_planes(case)
    want = _ref_corr(h, size, halo, Hy2, n_fc, n_cf, MASK_VALUE)
    rows = 8
    for b in range(3):
        lo = b * rows                                              # 0-based padded row of the band's row jstart - Hy
        cut = {k: np.ascontiguousarray(h[k][:, lo:lo + rows + 2 * Hy, :]) for k in FIELDS}
        cut.update({k: np.ascontiguousarray(h[k][lo:lo + rows + 2 * Hy2, :]) for k in PLANES})
        cut["dz_c"], cut["depth"] = h["dz_c"], h["depth"]
        bn = [np.ascontiguousarray(n[lo:lo + rows]) for n in (n_fc, n_cf)]
        bsize = (Nx, rows, Nz)
        got = _mode(osg, gpu, cut, bsize, halo, Hy2)
        for q, k in enumerate(("want_Ubar", "want_Vbar")):
            _assert_same(got[q][Hy2:Hy2 + rows, Hx:Hx + Nx], h[k][Hy2 + lo:Hy2 + lo + rows, Hx:Hx + Nx], ("band mode", b, q))
        for q, w in enumerate(_ref_mode(cut, bsize, halo, Hy2)):
            _assert_same(got[q], w, ("band mode plane", b, q))
        got = _corr(osg, gpu, cut, bsize, halo, Hy2, "both", *bn, MASK_VALUE)
        for q in range(2):
            _assert_same(got[q][Hz:Hz + Nz, Hy:Hy + rows, Hx:Hx + Nx], want[q][Hz:Hz + Nz, Hy + lo:Hy + lo + rows, Hx:Hx + Nx], ("band correction", b, q))
        for q, w in enumerate(_ref_corr(cut, bsize, halo, Hy2, *bn, MASK_VALUE)):
            _assert_same(got[q], w, ("band correction parent", b, q))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_exactness_identity_on_the_device(osg, gpu, dtype):
    """integer u, v and power-of-two dz_c through the C ABI: Ubar is the exact integer sum; after the correction with an integer U and
    H = sum dz_c a power of two, the mode of the corrected velocities IS U, exactly"""
    size, halo, Hy2 = (20, 12, 4), (2, 2, 1), 3
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = _shapes(size, halo, Hy2)
    rng = np.random.default_rng(9)
    h = {k: rng.integers(-9, 10, parent).astype(dtype) for k in FIELDS}
    h["dz_c"] = np.array([1, 2, 4, 1], dtype)                      # sum 8
    h["depth"] = np.array([8, 7, 5, 1, 0], dtype)
    ubar, vbar = _mode(osg, gpu, h, size, halo, Hy2)
    for got, f in ((ubar, h["u"]), (vbar, h["v"])):
        exact = (h["dz_c"].astype(np.int64)[:, None, None] * f[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx].astype(np.int64)).sum(0)
        assert np.array_equal(got[Hy2:Hy2 + Ny, Hx:Hx + Nx].astype(np.int64), exact) and np.array_equal(got[Hy2:Hy2 + Ny, Hx:Hx + Nx], exact.astype(dtype))
    h["Ubar"], h["Vbar"] = ubar, vbar
    h["U"], h["V"] = rng.integers(-64, 65, plane).astype(dtype), rng.integers(-64, 65, plane).astype(dtype)
    h["u"], h["v"] = _corr(osg, gpu, h, size, halo, Hy2)
    again = _mode(osg, gpu, h, size, halo, Hy2)
    for got, k in zip(again, ("U", "V")):
        _assert_same(got[Hy2:Hy2 + Ny, Hx:Hx + Nx], h[k][Hy2:Hy2 + Ny, Hx:Hx + Nx], ("mode of the corrected", k))


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
HY_EXT = 13                                                        # the extended north halo of 12 sub-steps


def _grid_fields(osg, gpu, size, halo, tdt, grid=None, seed=3):
    """(grid, the extended-halo grid of the 2-D fields, u, v with random data in every cell)"""
    base = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0)) if grid is None else getattr(grid, "underlying_grid", grid)
    grid = base if grid is None else grid
    ext = osg.with_halo((halo[0], HY_EXT, halo[2]), base)
    gen = torch.Generator(device=gpu).manual_seed(seed)
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v):
        f.data.uniform_(-1, 1, generator=gen)
    return grid, ext, u, v


def _planes(osg, gpu, ext, seed=4, names=("U", "V")):
    gen = torch.Generator(device=gpu).manual_seed(seed)
    out = []
    for name in names:
        f = osg.Field((osg.Face, osg.Center, None) if name[0] == "U" else (osg.Center, osg.Face, None), ext, name=name)
        f.data.uniform_(-1, 1, generator=gen)
        out.append(f)
    return out


def _np_type(tdt):
    return F64 if tdt == torch.float64 else F32


def _grid_mode_ref(osg, grid, f, size, halo):
    """the interior (Ny, Nx) of the mode of the field f from its host copy and the grid's own z_center_spacings"""
    host = f.data.cpu().numpy()
    dz = osg.z_center_spacings(grid, f.data.dtype).numpy().astype(host.dtype)
    return ref.interior_mode(host, dz, size, halo)


def _grid_corr_ref(osg, grid, f, t, tbar, size, halo, n=None):
    """the corrected interior (Nz, Ny, Nx) of the field f from host copies and the grid's own column_depth_table"""
    host = f.data.cpu().numpy()
    depth = osg.column_depth_table(grid, f.data.dtype).numpy().astype(host.dtype)
    return ref.interior_correction(host, t.data[0].cpu().numpy(), tbar.data[0].cpu().numpy(), depth, size, halo, t.Hy, n, 0.0)


def _filled(osg, like, interior, grid, base=None):
    """the parent fill_halo_regions gives a field at `like`'s location that held `base` (a parent: tensor or array; None: zeros) and got
    that interior"""
    f = osg.Field(like.loc, grid)
    if base is not None:
        f.data.copy_(torch.as_tensor(base).reshape(f.data.shape))
    f.interior().copy_(torch.from_numpy(np.ascontiguousarray(interior)).reshape(f.interior().shape))
    osg.fill_halo_regions([f])
    return f.data.cpu().numpy()


PACKAGE = [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)]


@pytest.mark.parametrize("size,halo,tdt", PACKAGE, ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_mode_and_correction_on_a_built_grid(osg, gpu, size, halo, tdt):
    """u, v on a built grid, the 2-D fields on with_halo((Hx, 13, Hz), grid): the interiors equal the reference from the grid's own
    z_center_spacings / column_depth_table; with fill_halos the parents are what fill_halo_regions gives fields with that interior (U, V:
    the sign-flipping zipper into all 13 north rows), without it the halos stay as they were"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, ext, u, v = _grid_fields(osg, gpu, size, halo, tdt)
    want = [_grid_mode_ref(osg, grid, f, size, halo) for f in (u, v)]
    Ub, Vb = _planes(osg, gpu, ext, names=("Ubar", "Vbar"))
    held = [f.data.clone() for f in (Ub, Vb)]                      # random in every cell: the south halo has no condition and keeps it
    got = osg.compute_barotropic_mode(u, v, Ub, Vb)
    assert got[0] is Ub and got[1] is Vb and Ub.Hy == HY_EXT and tuple(Ub.data.shape) == (1, Ny + 2 * HY_EXT, Nx + 2 * Hx)
    for f, w, b in zip((Ub, Vb), want, held):                      # the fold also takes the east half of interior row Ny, as in every filled field
        _assert_same(f.data.cpu().numpy(), _filled(osg, f, w, ext, b), "mode: filled halos")
    north = Ub.data[0, HY_EXT + Ny:, Hx:Hx + Nx]
    assert north.shape[0] == HY_EXT and bool((north != 0).all())   # all 13 north rows written
    # allocated outputs live on the fields' own grid; one pair alone
    U0, V0 = osg.compute_barotropic_mode(u, v)
    assert U0.grid is grid and U0.loc == (osg.Face, osg.Center, None) and V0.loc == (osg.Center, osg.Face, None) and U0.Hy == Hy
    _assert_same(U0.data.cpu().numpy(), _filled(osg, U0, want[0], grid), "allocated U")
    _assert_same(V0.data.cpu().numpy(), _filled(osg, V0, want[1], grid), "allocated V")
    none, V1 = osg.compute_barotropic_mode(None, v)
    assert none is None
    _assert_same(V1.data.cpu().numpy(), V0.data.cpu().numpy(), "v alone")
    # halos left alone
    Us, Vs = _planes(osg, gpu, ext)
    for f in (Us, Vs):
        f.data.fill_(SENTINEL)
    plan = osg.barotropic_mode_plan(u, v, Us, Vs, fill_halos=False)
    assert plan() is plan and plan.U is Us and plan.V is Vs
    for f, w in zip((Us, Vs), want):
        bare = np.full(tuple(f.data.shape), SENTINEL, w.dtype)
        bare[0, HY_EXT:HY_EXT + Ny, Hx:Hx + Nx] = w
        _assert_same(f.data.cpu().numpy(), bare, "mode: halos left alone")
    # the correction, with the mode given and with the plan's own
    U, V = _planes(osg, gpu, ext)
    want_u, want_v = _grid_corr_ref(osg, grid, u, U, Ub, size, halo), _grid_corr_ref(osg, grid, v, V, Vb, size, halo)
    before = [f.data.clone() for f in (u, v)]
    u2, v2 = (osg.Field(f.loc, grid, data=f.data.clone()) for f in (u, v))
    assert osg.barotropic_correction_plan(u2, v2, U, V, Ub, Vb, fill_halos=False)().u is u2
    for f, w, b in zip((u2, v2), (want_u, want_v), before):
        bare = b.cpu().numpy()
        bare[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = w
        _assert_same(f.data.cpu().numpy(), bare, "correction: halos left alone")
    # Ubar, Vbar computed first, into the plan's own planes: the mode as the rule leaves it (Us, Vs above), no fill in between
    want_u, want_v = _grid_corr_ref(osg, grid, u, U, Us, size, halo), _grid_corr_ref(osg, grid, v, V, Vs, size, halo)
    got = osg.barotropic_correction(u, v, U, V)
    assert got[0] is u and got[1] is v
    for f, w, b in zip((u, v), (want_u, want_v), before):
        _assert_same(f.data.cpu().numpy(), _filled(osg, f, w, grid, b), "correction: filled halos")


def test_plans_replay_in_a_graph_and_allocate_nothing(osg, gpu):
    size, halo = (48, 40, 6), (4, 4, 4)
    grid, ext, u, v = _grid_fields(osg, gpu, size, halo, torch.float64)
    U, V = _planes(osg, gpu, ext)
    Ub, Vb = _planes(osg, gpu, ext, names=("Ubar", "Vbar"))
    mode = osg.barotropic_mode_plan(u, v, Ub, Vb)
    corr = osg.barotropic_correction_plan(u, v, U, V, Ub, Vb)
    own = osg.barotropic_correction_plan(u, v, U, V)
    assert mode() is mode and corr() is corr and own() is own      # eager warm-up (first-call work outside the capture)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    mode(); corr(); own()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            mode()
            corr()
    torch.cuda.current_stream().wait_stream(side)
    gen = torch.Generator(device=gpu).manual_seed(17)
    for _ in range(2):                                             # u changes, the graph is replayed: the results are the references'
        u.data.uniform_(-1, 1, generator=gen)
        want_bar = [_grid_mode_ref(osg, grid, f, size, halo) for f in (u, v)]
        host_u, host_v = u.data.cpu().numpy(), v.data.cpu().numpy()
        Ub.data.zero_()
        Vb.data.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for f, w in zip((Ub, Vb), want_bar):
            _assert_same(f.data.cpu().numpy(), _filled(osg, f, w, ext), "replay: mode")
        depth = osg.column_depth_table(grid, torch.float64).numpy()
        for f, host, t, tb in ((u, host_u, U, Ub), (v, host_v, V, Vb)):
            w = ref.interior_correction(host, t.data[0].cpu().numpy(), tb.data[0].cpu().numpy(), depth, size, halo, HY_EXT)
            _assert_same(f.data.cpu().numpy(), _filled(osg, f, w, grid, host), "replay: correction")


def test_immersed_grid_masks_the_peripheral_nodes_in_the_same_call(osg, gpu):
    """on an ImmersedBoundaryGrid the count planes go into the call: H is the column's own depth and the peripheral nodes get 0.  With
    mask_immersed=False no plane goes in and H is the full depth in every column, so the equality with the mask pass afterwards is held on
    a bottom of open and land columns only (a wall), where H is the same wherever a node survives the mask"""
    size, halo = (48, 40, 6), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    base = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo, z=(-1, 0))
    zc = base.z_centers[Hz:Hz + Nz].cpu().numpy()
    rng = np.random.default_rng(19)
    drawn = draw_columns(rng, Nx, Ny, Nz)
    for wall in (False, True):
        columns = np.where(drawn >= Nz // 2, Nz, 0).astype(drawn.dtype) if wall else drawn
        ibg = osg.ImmersedBoundaryGrid(base, osg.GridFittedBottom(heights_of(columns, zc, rng)))
        _, ext, u, v = _grid_fields(osg, gpu, size, halo, torch.float64, grid=ibg)
        U, V = _planes(osg, gpu, ext)
        Ub, Vb = _planes(osg, gpu, ext, names=("Ubar", "Vbar"))
        nfc, ncf = (ibg.column_counts[k].cpu().numpy() for k in ("fc", "cf"))
        assert (nfc >= Nz).any() and (nfc == 0).any() and (wall != bool(((nfc > 0) & (nfc < Nz)).any()))
        want_u, want_v = _grid_corr_ref(osg, ibg, u, U, Ub, size, halo, nfc), _grid_corr_ref(osg, ibg, v, V, Vb, size, halo, ncf)
        raw_u, raw_v = _grid_corr_ref(osg, ibg, u, U, Ub, size, halo), _grid_corr_ref(osg, ibg, v, V, Vb, size, halo)
        u1, v1 = (osg.Field(f.loc, ibg, data=f.data.clone()) for f in (u, v))
        u2, v2 = (osg.Field(f.loc, ibg, data=f.data.clone()) for f in (u, v))
        osg.barotropic_correction(u1, v1, U, V, Ub, Vb, fill_halos=False)
        _assert_same(u1.interior().cpu().numpy(), want_u, "masked u")
        _assert_same(v1.interior().cpu().numpy(), want_v, "masked v")
        assert not bool(u1.interior().isnan().any()) and bool((u1.interior()[:, torch.from_numpy(nfc >= Nz).to(gpu)] == 0).all())
        osg.barotropic_correction(u, v, U, V, Ub, Vb)
        osg.barotropic_correction(u2, v2, U, V, Ub, Vb, mask_immersed=False, fill_halos=False)
        _assert_same(u2.interior().cpu().numpy(), raw_u, "unmasked u")
        _assert_same(v2.interior().cpu().numpy(), raw_v, "unmasked v")
        if wall:
            osg.mask_immersed_field([u2, v2], 0)
            osg.fill_halo_regions([u2, v2])
            _assert_same(u2.data.cpu().numpy(), u.data.cpu().numpy(), "u: mask pass + fill")
            _assert_same(v2.data.cpu().numpy(), v.data.cpu().numpy(), "v: mask pass + fill")


def test_a_full_step_against_the_three_references_chained(osg, gpu):
    """compute_barotropic_mode -> the sub-cycle's stand-in (U, V perturbed) -> barotropic_correction -> compute_w_from_continuity"""
    size, halo = (48, 40, 6), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, ext, u, v = _grid_fields(osg, gpu, size, halo, torch.float64)
    host = {"u": u.data.cpu().numpy(), "v": v.data.cpu().numpy()}
    Ub, Vb = _planes(osg, gpu, ext, names=("Ubar", "Vbar"))
    held = [f.data.clone() for f in (Ub, Vb)]
    osg.compute_barotropic_mode(u, v, Ub, Vb)
    U, V = _planes(osg, gpu, ext)
    for t, tb in ((U, Ub), (V, Vb)):
        t.data.mul_(0.01).add_(tb.data)
    osg.barotropic_correction(u, v, U, V, Ub, Vb)
    w = osg.compute_w_from_continuity(u, v)
    # the references, chained on the host
    dz = osg.z_center_spacings(grid, torch.float64).numpy()
    depth = osg.column_depth_table(grid, torch.float64).numpy()
    bar = {k: ref.interior_mode(host[k], dz, size, halo) for k in FIELDS}
    _assert_same(Ub.data.cpu().numpy(), _filled(osg, Ub, bar["u"], ext, held[0]), "step: Ubar")
    _assert_same(Vb.data.cpu().numpy(), _filled(osg, Vb, bar["v"], ext, held[1]), "step: Vbar")
    filled = {}
    for k, f, t, tb in (("u", u, U, Ub), ("v", v, V, Vb)):
        c = ref.interior_correction(host[k], t.data[0].cpu().numpy(), tb.data[0].cpu().numpy(), depth, size, halo, HY_EXT)
        filled[k] = _filled(osg, f, c, grid, host[k])
        _assert_same(f.data.cpu().numpy(), filled[k], ("step: corrected", k))
    metrics = [grid.arrays[k].cpu().numpy() for k in ("dy_fc", "dx_cf", "az_cc")]
    want_w, _ = interior_w_and_divergence(filled["u"], filled["v"], *metrics, dz, size, halo)
    _assert_same(w.interior().cpu().numpy(), want_w, "step: w")


# ---- past 2^31 elements --------------------------------------------------------------------------------------------------------------------
def test_float32_past_2g_elements(osg, gpu):
    """8640 x 4320 x 64, halo 4, Float32, u only (v, Vbar NULL): 2.7e9 elements in the parent, so the element offsets of the upper levels
    need 64 bits.  u = 0 below the top two levels, drawn on the device above: Ubar is compared in full with numpy on the two top slabs (the
    sum arrives there as +0).  Then the correction with a device-drawn U: the top two levels and level 1 are compared in full, three halo
    rings and both halo slabs stay as they were"""
    size, halo, Hy2 = (8640, 4320, 64), (4, 4, 4), 4
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = _shapes(size, halo, Hy2)
    assert parent[0] * parent[1] * parent[2] > 1 << 31
    lib = osg._lib.barotropic_lib()
    gen = torch.Generator(device=gpu).manual_seed(5)
    u = torch.full(parent, SENTINEL, dtype=torch.float32, device=gpu)
    u[Hz:Hz + Nz - 2, Hy:Hy + Ny, Hx:Hx + Nx] = 0
    top = slice(Hz + Nz - 2, Hz + Nz)                              # parent planes of levels Nz - 1 and Nz
    inner2 = (slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    u[top][:, inner2[0], inner2[1]] = torch.empty((2, Ny, Nx), dtype=torch.float32, device=gpu).uniform_(-1, 1, generator=gen)
    dz = torch.empty(Nz, dtype=torch.float32, device=gpu).uniform_(0.5, 2, generator=gen)
    depth = torch.empty(Nz + 1, dtype=torch.float32, device=gpu).uniform_(0.5, 2, generator=gen)
    Ubar = torch.full(plane, SENTINEL, dtype=torch.float32, device=gpu)
    U = torch.empty(plane, dtype=torch.float32, device=gpu).uniform_(-1, 1, generator=gen)
    stream = osg._lib.current_stream_ptr(gpu)
    osg._lib.check_barotropic(lib.tpg_barotropic_mode(u.data_ptr(), None, Ubar.data_ptr(), None, dz.data_ptr(), *size, *halo, Hy2,
                                                      osg._lib.TPG_F32, stream))
    torch.cuda.synchronize()
    slab = u[top][:, inner2[0], inner2[1]].cpu().numpy()
    hdz = dz.cpu().numpy()
    want = np.full(plane, SENTINEL, F32)
    want[inner2] = (F32(0) + hdz[Nz - 2] * slab[0]) + hdz[Nz - 1] * slab[1]
    host_ubar = Ubar.cpu().numpy()
    _assert_same(host_ubar, want, "Ubar")
    assert np.isfinite(want).all() and (want[inner2] != 0).mean() > 0.99
    # the correction
    osg._lib.check_barotropic(lib.tpg_barotropic_correction(u.data_ptr(), None, U.data_ptr(), None, Ubar.data_ptr(), None, depth.data_ptr(),
                                                            None, None, 0.0, *size, *halo, Hy2, osg._lib.TPG_F32, stream))
    torch.cuda.synchronize()
    c = (U.cpu().numpy()[inner2] - host_ubar[inner2]) / depth.cpu().numpy()[0]
    assert (c != 0).mean() > 0.99
    _assert_same(u[top][:, inner2[0], inner2[1]].cpu().numpy(), slab + c[None], "top levels")
    _assert_same(u[Hz][inner2].cpu().numpy(), F32(0) + c, "level 1")
    # every halo cell as it was: the rows and columns round three interior levels, and both halo slabs
    edge = torch.ones(parent[1:], dtype=torch.bool, device=gpu)
    edge[inner2] = False
    for k in (Hz, Hz + Nz // 2, Hz + Nz - 1):
        assert bool((u[k][edge] == SENTINEL).all()), k
    assert bool((u[:Hz] == SENTINEL).all()) and bool((u[Hz + Nz:] == SENTINEL).all())
