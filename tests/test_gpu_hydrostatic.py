"""GPU tests of the Coriolis and hydrostatic pressure-gradient tendencies: tpg_hydrostatic_tendencies through the C ABI, and
hydrostatic_tendencies_plan / update_hydrostatic_pressure through the package.  Compared BIT FOR BIT with tests/hydrostatic_ref.py (numpy in
the fields' type: every operation of the rule is one correctly rounded IEEE operation, so the reference is exact and there is no tolerance
anywhere in this file); NaNs compare by NaN-ness; whole parents are compared: the halo cells of Gu, Gv and p_out against what they held (a
sentinel in WRITE mode and in p_out, the random start in ADD mode), and the inputs must come back unchanged.

Shapes: the momentum test's list, the smallest at which each path can go wrong -- the smallest served shape (one chunk, one row, one level);
one level (only the top step); two levels at the minimum halo; the minimum halo in both types (every arm and both corners end on the last
halo cell); odd Hx (the element-aligned chunks), also with every pointer one element off the 16-B grid; more levels than twice the
look-ahead and no multiple of it; an odd Ny (a partial last row tile) on Float32 rows that sit on the 16-B grid; the model halo 5; Float32
with Nx = 2 mod 4 (8-B chunks); one shape with more work items than are resident.  The committed kernel takes 2 rows per item in Float64 and 1
in Float32, look-ahead 1 in both: the partial last row tile exists in Float64 only, so 24 x 11 x 5 is here in Float64 too (and 2 x 1 x 1 and
2304 x 1283 x 2 are partial tiles as well), while its Float32 case keeps the rows on the 16-B grid with an odd Ny for the measured 2-row
Float32 variant; 9 and 5 levels are more than twice the look-ahead of the committed and of the measured look-ahead-2 form and no multiple of
either.  dz_f is random in [0.5, 2] and f_ff random in [-1, 1], so a wrong face index or a wrong corner cannot hide."""
import ctypes as C

import numpy as np
import pytest
import torch

import hydrostatic_ref as R
import momentum_ref
from gpu_harness import F32, F64, MASK_VALUE, SENTINEL, _assert_parent, _count_planes, _dev, _free_hbm, _id  # noqa: F401
from hydrostatic_ref import ADD, ENERGY, ENSTROPHY, WRITE, same_bits
from special_values import pool

pytestmark = pytest.mark.gpu

#         size            halo       element type
SMALL = [((2, 1, 1), (1, 1, 1), F64),              # the smallest served shape: one chunk, one row, one level
         ((10, 10, 1), (4, 4, 4), F64),            # only the top step
         ((20, 12, 2), (1, 1, 1), F32),            # two levels at the minimum halo
         ((20, 12, 3), (1, 1, 1), F64),            # every arm and both corners end on the last halo cell
         ((20, 12, 3), (1, 1, 1), F32),
         ((20, 12, 3), (3, 2, 1), F64),            # odd Hx: the element-aligned chunks
         ((20, 10, 9), (4, 4, 4), F64),            # more levels than twice the look-ahead and no multiple of it
         ((24, 11, 5), (4, 4, 4), F32),            # Ny odd, rows on the 16-B grid (a partial last row tile of the 2-row Float32 variant)
         ((48, 40, 6), (5, 5, 5), F64),            # the model halo
         ((48, 40, 6), (5, 5, 5), F32),
         ((50, 40, 3), (4, 4, 4), F32),            # Nx = 2 mod 4: 8-B chunks
         ((24, 11, 5), (4, 4, 4), F64)]            # Ny odd: a partial last row tile (2 rows per item in Float64)
BIG = ((2304, 1283, 2), (4, 4, 4), F64)            # 642 row tiles x 1152 chunks, more items than are resident; the last tile partial
OFFSET = [SMALL[5], SMALL[6], SMALL[10]]           # every pointer one element off the 16-B grid: the GEN form by the pointers, not the rows
FIELDS = ("u", "v", "b", "Gu0", "Gv0")
PLANES = ("f_ff", *R.METRICS)

# a form: (Coriolis scheme or None, pressure term, mode, p_out given, Gu and Gv given)
FORMS = {"full-add": (ENSTROPHY, True, ADD, False, True), "full-write": (ENSTROPHY, True, WRITE, False, True),
         "energy-add": (ENERGY, True, ADD, False, True), "energy-write": (ENERGY, True, WRITE, False, True),
         "coriolis-add": (ENSTROPHY, False, ADD, False, True), "coriolis-energy-write": (ENERGY, False, WRITE, False, True),
         "pressure-add": (None, True, ADD, False, True), "pressure-write": (None, True, WRITE, False, True),
         "full-add-p": (ENSTROPHY, True, ADD, True, True), "energy-write-p": (ENERGY, True, WRITE, True, True),
         "p-alone": (None, True, WRITE, True, False)}
MORE = {"coriolis-write": (ENSTROPHY, False, WRITE, False, True)}      # beside FORMS, for the test of ADD onto -0
# every form meets the smallest shape and one multi-level shape (the last of each row, sparsely spread); every shape meets the full form
CROSS = ([(c, "full-add", 0) for c in SMALL] + [(c, "full-add", 1) for c in OFFSET] + [(SMALL[0], f, 0) for f in FORMS if f != "full-add"]
         + [(c, f, 0) for c, f in zip((SMALL[3], SMALL[7], SMALL[6], SMALL[9], SMALL[10], SMALL[4], SMALL[8], SMALL[5], SMALL[7], SMALL[6]),
                                      [f for f in FORMS if f != "full-add"])]
         + [(SMALL[10], "energy-write-p", 1), (SMALL[5], "p-alone", 1)])

_CASES = {}


def _case(case):
    """host arrays of a case, random in EVERY cell (halos included): u, v, b, the start of Gu and Gv and f_ff in [-1, 1], the metrics and dz_f
    in [0.5, 2].  Drawn once per case, shared by the tests, never modified (tests copy what they change)"""
    if case not in _CASES:
        size, halo, dtype = case
        (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
        rng = np.random.default_rng([5, *size, *halo, np.dtype(dtype).itemsize])
        parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
        h = {k: rng.uniform(-1, 1, parent).astype(dtype) for k in FIELDS}
        h["f_ff"] = rng.uniform(-1, 1, plane).astype(dtype)
        for k in R.METRICS:
            h[k] = rng.uniform(0.5, 2, plane).astype(dtype)
        h["dz_f"] = rng.uniform(0.5, 2, Nz + 1).astype(dtype)
        for a in h.values():
            a.setflags(write=False)
        _CASES[case] = h
    return _CASES[case]


_WANT = {}


def _ref(h, size, halo, form, n_fc=None, n_cf=None, key=None):
    """the reference parents (Gu, Gv, p) of a form: WRITE starts from sentinel-filled Gu, Gv; ADD from h's; p_out from a sentinel-filled one"""
    if key is not None and (key, form) in _WANT:
        return _WANT[key, form]
    scheme, pres, mode, p_out, hasG = {**FORMS, **MORE}[form]
    dtype = h["u"].dtype.type
    sent = np.full(h["u"].shape, SENTINEL, dtype)
    Gu0, Gv0 = ((h["Gu0"], h["Gv0"]) if mode == ADD else (sent, sent)) if hasG else (None, None)
    with np.errstate(all="ignore"):
        want = R.tendencies(h["u"], h["v"], h["b"] if pres else None, Gu0, Gv0, sent if p_out else None, None if scheme is None else h["f_ff"],
                            h, h["dz_f"], size, halo, scheme or 0, mode, n_fc, n_cf, MASK_VALUE)
    if key is not None:
        _WANT[key, form] = want
    return want


def _raw(osg, gpu, d, Gu, Gv, p, size, halo, scheme=0, mode=ADD, cor=True, pres=True, n_fc=None, n_cf=None, value=MASK_VALUE, over=None):
    """the status of tpg_hydrostatic_tendencies on the device arrays d; a dropped term passes NULL for everything only it reads"""
    ptr = lambda t: None if t is None else t.data_ptr()           # noqa: E731
    a = dict(u=d["u"] if cor else None, v=d["v"] if cor else None, b=d["b"] if pres else None, Gu=Gu, Gv=Gv, p=p,
             f_ff=d["f_ff"] if cor else None, dx_fc=d["dx_fc"] if Gu is not None else None, dy_fc=d["dy_fc"] if cor else None,
             dx_cf=d["dx_cf"] if cor else None, dy_cf=d["dy_cf"] if Gu is not None else None, dz_f=d["dz_f"] if pres else None,
             n_fc=n_fc, n_cf=n_cf)
    a.update(over or {})
    lib = osg._lib
    return lib.hydrostatic_lib().tpg_hydrostatic_tendencies(*(ptr(t) for t in a.values()), value, scheme, mode, *size, *halo,
                                                           lib.ft_of(d["dz_f"].dtype if pres else d["f_ff"].dtype), lib.current_stream_ptr(gpu))


def _device(h, gpu, offset=0):
    return {k: _dev(a, gpu, offset) for k, a in h.items() if k not in ("Gu0", "Gv0")}


def _call(osg, gpu, d, h, size, halo, form, offset=0, n_fc=None, n_cf=None):
    """the entry point in a form on the device arrays d -> the whole parents (Gu, Gv, p) on the host (None where the form has none)"""
    scheme, pres, mode, p_out, hasG = {**FORMS, **MORE}[form]
    dtype = h["u"].dtype.type
    sent = np.full(h["u"].shape, SENTINEL, dtype)
    Gu = Gv = p = None
    if hasG:
        Gu, Gv = (_dev(h[k] if mode == ADD else sent, gpu, offset) for k in ("Gu0", "Gv0"))
    if p_out:
        p = _dev(sent, gpu, offset)
    osg._lib.check_hydrostatic(_raw(osg, gpu, d, Gu, Gv, p, size, halo, scheme or 0, mode, scheme is not None, pres, n_fc, n_cf))
    return tuple(None if t is None else t.cpu().numpy() for t in (Gu, Gv, p))


def _assert_triple(got, want, what):
    for name, g, w_ in zip(("Gu", "Gv", "p"), got, want):
        assert (g is None) == (w_ is None), (what, name)
        if g is not None:
            _assert_parent(g, w_, (what, name))


def _assert_unchanged(d, h, what):
    for k, t in d.items():
        _assert_parent(t.cpu().numpy(), h[k], (what, "input", k))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,form,offset", CROSS, ids=[f"{_id(c)}-{f}" + ("-offset" if o else "") for c, f, o in CROSS])
def test_interior_is_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, form, offset):
    """random data in every cell: the whole parents equal the reference's -- the interior the rule, every halo cell what it held -- and
    every input comes back as it was"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    want = _ref(h, size, halo, form, key=case)
    for w_ in want:
        if w_ is not None:
            inner = w_[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
            assert np.isfinite(w_).all() and not (inner == SENTINEL).any()
    d = _device(h, gpu, offset)
    _assert_triple(_call(osg, gpu, d, h, size, halo, form, offset), want, form)
    _assert_unchanged(d, h, form)


def test_more_items_than_are_resident(osg, gpu):
    size, halo, dtype = BIG
    h = _case(BIG)
    d = _device(h, gpu)
    _assert_triple(_call(osg, gpu, d, h, size, halo, "full-add-p"), _ref(h, size, halo, "full-add-p"), "big")


@pytest.mark.parametrize("case,form,offset", [(SMALL[0], "full-add", 0), (SMALL[3], "full-add", 0), (SMALL[7], "energy-write", 0),
                                              (SMALL[5], "full-add-p", 1), (SMALL[9], "coriolis-add", 0), (SMALL[6], "pressure-write", 0),
                                              (SMALL[10], "p-alone", 0)], ids=lambda x: x if isinstance(x, str) else None)
def test_no_cell_outside_the_stencil_is_read(osg, gpu, case, form, offset):
    """every cell of u, v, b, f_ff and the four metric planes that cells_read says the form does not read is NaN: the result has no NaN and
    equals the clean one"""
    size, halo, dtype = case
    scheme, pres, mode, p_out, hasG = FORMS[form]
    h = _case(case)
    read = R.cells_read(size, halo, scheme is not None, pres, "both" if hasG else "p")
    poisoned = dict(h, **{k: np.where(read[k], h[k], dtype(np.nan)) for k in read})
    assert all(np.isnan(poisoned[k]).sum() == (~read[k]).sum() > 0 for k in read)
    got = _call(osg, gpu, _device(poisoned, gpu, offset), h, size, halo, form, offset)
    assert not any(np.isnan(g).any() for g in got if g is not None)
    _assert_triple(got, _ref(h, size, halo, form, key=case), "poisoned")


@pytest.mark.parametrize("case,form,offset", [(SMALL[3], "full-add", 0), (SMALL[7], "energy-write-p", 0), (SMALL[5], "full-write", 1),
                                              (SMALL[9], "pressure-add", 0), (SMALL[10], "coriolis-add", 0)],
                         ids=lambda x: x if isinstance(x, str) else None)
def test_fused_mask_equals_the_reference_and_the_mask_pass(osg, gpu, case, form, offset):
    """with the count planes: (1) the reference with the mask, in both modes, p_out unmasked; (2) the unmasked call followed by
    tpg_mask_immersed_fields on Gu (by n_fc) and Gv (by n_cf), bit for bit on the whole parents"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    nfc, ncf = _count_planes(case)
    want, unmasked = _ref(h, size, halo, form, nfc, ncf), _ref(h, size, halo, form, key=case)
    assert same_bits(want[0], unmasked[0]) > 0 and same_bits(want[1], unmasked[1]) > 0
    d = _device(h, gpu, offset)
    nd = [_dev(nfc, gpu, offset), _dev(ncf, gpu, offset)]
    _assert_triple(_call(osg, gpu, d, h, size, halo, form, offset, *nd), want, "fused mask")
    t = [_dev(unmasked[q], gpu, offset) for q in (0, 1)]
    L = osg._lib
    L.check(L.lib().tpg_mask_immersed_fields(L.ptr_table(t), 2, L.ptr_table(nd), (C.c_int8 * 2)(L.TPG_CENTER, L.TPG_CENTER),
                                             (C.c_double * 2)(MASK_VALUE, MASK_VALUE), Nx, Ny, Nz, *halo, L.ft_of(t[0].dtype),
                                             L.current_stream_ptr(gpu)))
    for q in (0, 1):
        _assert_parent(t[q].cpu().numpy(), want[q], ("two passes", q))


@pytest.mark.parametrize("case", [SMALL[4], SMALL[8]], ids=_id)
@pytest.mark.parametrize("scheme", ["full", "energy", "coriolis", "pressure"])
def test_add_onto_minus_zero_is_write(osg, gpu, case, scheme):
    """-0 is the additive identity: ADD onto Gu = Gv = -0 gives WRITE's bits, on the device as in the reference"""
    size, halo, dtype = case
    add, write = {"full": ("full-add", "full-write"), "energy": ("energy-add", "energy-write"),
                  "coriolis": ("coriolis-add", "coriolis-write"), "pressure": ("pressure-add", "pressure-write")}[scheme]
    h = dict(_case(case))
    h["Gu0"] = h["Gv0"] = np.full(h["u"].shape, -0.0, dtype)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    d = _device(h, gpu)
    got_add, got_write = _call(osg, gpu, d, h, size, halo, add), _call(osg, gpu, d, h, size, halo, write)
    for q in (0, 1):
        assert same_bits(got_add[q][cut], got_write[q][cut]) == 0
        _assert_parent(got_write[q], _ref(_case(case), size, halo, write, key=case)[q], "write")


def test_add_after_the_advection_call(osg, gpu):
    """ADD onto what tpg_momentum_advection_tendency left in Gu, Gv equals the reference's ((-adv) + cu) - px, ((-adv) - cv) - py"""
    case = SMALL[8]
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = dict(_case(case))
    rng = np.random.default_rng(23)
    m = dict(h, **{k: rng.uniform(0.5, 2, h["dx_fc"].shape).astype(dtype) for k in ("az_fc", "az_cf", "az_cc", "az_ff")})
    w = rng.uniform(-1, 1, (Nz + 1 + 2 * Hz, *h["u"].shape[1:])).astype(dtype)
    sent = np.full(h["u"].shape, SENTINEL, dtype)
    with np.errstate(all="ignore"):
        adv = momentum_ref.tendencies(h["u"], h["v"], w, sent, sent, m, h["dz_f"], size, halo)
    d = _device(h, gpu)
    Gu, Gv, dw = _dev(sent, gpu), _dev(sent, gpu), _dev(w, gpu)
    dm = {k: _dev(m[k], gpu) for k in momentum_ref.METRICS}
    L = osg._lib
    L.check_momentum(L.momentum_lib().tpg_momentum_advection_tendency(
        d["u"].data_ptr(), d["v"].data_ptr(), dw.data_ptr(), Gu.data_ptr(), Gv.data_ptr(), *(dm[k].data_ptr() for k in momentum_ref.METRICS),
        d["dz_f"].data_ptr(), None, None, 0.0, 0, *size, *halo, L.ft_of(Gu.dtype), L.current_stream_ptr(gpu)))
    L.check_hydrostatic(_raw(osg, gpu, d, Gu, Gv, None, size, halo))
    h["Gu0"], h["Gv0"] = adv
    want = _ref(h, size, halo, "full-add")
    _assert_parent(Gu.cpu().numpy(), want[0], "Gu after advection")
    _assert_parent(Gv.cpu().numpy(), want[1], "Gv after advection")


def test_three_latitude_bands_give_the_rows_of_the_global_call(osg, gpu):
    """rows 1..8, 9..16 and 17..24 of a 24-row problem as calls of their own on the band's rows with Hy halo rows either side (filled: they
    are the global parent's rows): each band's interior rows are the global call's"""
    size, halo, dtype = (20, 24, 4), (3, 2, 2), F64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case((size, halo, dtype))
    whole = _ref(h, size, halo, "full-add-p", key=(size, halo, dtype))
    for j0 in (0, 8, 16):
        rows = slice(j0, j0 + 8 + 2 * Hy)
        band = {k: (a if a.ndim == 1 else np.ascontiguousarray(a[..., rows, :])) for k, a in h.items()}
        got = _call(osg, gpu, _device(band, gpu), band, (Nx, 8, Nz), halo, "full-add-p")
        for q in range(3):
            assert same_bits(got[q][Hz:Hz + Nz, Hy:Hy + 8, Hx:Hx + Nx], whole[q][Hz:Hz + Nz, Hy + j0:Hy + j0 + 8, Hx:Hx + Nx]) == 0, (j0, q)


@pytest.mark.parametrize("case,form", [(SMALL[8], "full-add"), (SMALL[9], "energy-write-p"), (SMALL[5], "full-write")],
                         ids=lambda x: x if isinstance(x, str) else None)
def test_special_values_in_read_cells(osg, gpu, case, form):
    """+-0, subnormals, +-Inf, NaN, +-max planted in 1 % of the cells of b, u, v and the start of Gu, Gv and 0.5 % of f_ff and each metric
    plane: bit for bit numpy's, which computes the same IEEE operations.  A special value in b reaches every level below it in three
    columns, so the finite share asserted is small"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    rng = np.random.default_rng([7, *size, *halo])
    p = pool(dtype)

    def plant(a, share):
        a = a.copy()
        where = rng.random(a.shape) < share
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
        return a

    planted = {k: plant(h[k], 0.01) for k in FIELDS}
    planted.update({k: plant(h[k], 0.005) for k in PLANES})
    planted["dz_f"] = h["dz_f"]
    planted["dx_fc"][Hy, Hx], planted["dy_cf"][Hy + 2, Hx + 2] = 0.0, -0.0
    planted["b"][Hz + Nz - 1, Hy + 1, Hx + 1], planted["u"][Hz, Hy + 3, Hx + 3], planted["f_ff"][Hy + 5, Hx + 5] = np.nan, np.inf, -0.0
    want = _ref(planted, size, halo, form)
    for G in want[:2]:
        inner = G[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(inner).any() and np.isinf(inner).any() and np.isfinite(inner).mean() > 0.1
    _assert_triple(_call(osg, gpu, _device(planted, gpu), planted, size, halo, form), want, "special values")


def test_domain_of_dependence_without_an_oracle(osg, gpu):
    """a bump in b at level k0 changes Gu, Gv only at levels <= k0 of its own column and of its east (Gu) and north (Gv) neighbours; a bump
    in f_ff changes only the header's nodes: Gu at (0,0), (0,-1) and Gv at (0,0), (-1,0) of every level"""
    case = SMALL[8]
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    base = _call(osg, gpu, _device(h, gpu), h, size, halo, "full-add")
    i, j, k0 = 17, 9, 4                                            # 1-based interior node
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]          # noqa: E731
    bumped = dict(h, b=h["b"].copy())
    bumped["b"][k0 + Hz - 1, j + Hy - 1, i + Hx - 1] += dtype(0.25)
    got = _call(osg, gpu, _device(bumped, gpu), bumped, size, halo, "full-add")
    for q, nodes in ((0, {(j, i), (j, i + 1)}), (1, {(j, i), (j + 1, i)})):
        changed = cut(got[q]) != cut(base[q])
        where = {(int(a), int(b_), int(c)) for a, b_, c in zip(*np.nonzero(changed))}
        assert where == {(k - 1, jj - 1, ii - 1) for k in range(1, k0 + 1) for jj, ii in nodes}, (q, sorted(where))
    bumped = dict(h, f_ff=h["f_ff"].copy())
    bumped["f_ff"][j + Hy - 1, i + Hx - 1] += dtype(0.25)
    got = _call(osg, gpu, _device(bumped, gpu), bumped, size, halo, "full-add")
    for q, nodes in ((0, {(j, i), (j - 1, i)}), (1, {(j, i), (j, i - 1)})):
        changed = cut(got[q]) != cut(base[q])
        where = {(int(a), int(b_), int(c)) for a, b_, c in zip(*np.nonzero(changed))}
        assert where == {(k - 1, jj - 1, ii - 1) for k in range(1, Nz + 1) for jj, ii in nodes}, (q, sorted(where))


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched, the outputs keep the sentinel"""
    case = SMALL[3]
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.hydrostatic_lib()
    err = lambda: lib.tpg_hydrostatic_last_error().decode()       # noqa: E731
    out = [_dev(np.full(h["u"].shape, SENTINEL, dtype), gpu) for _ in range(3)]
    assert _raw(osg, gpu, d, out[0], d["u"], None, size, halo) == -1 and err().startswith("Gv overlaps u")
    assert _raw(osg, gpu, d, out[0], out[1], d["b"], size, halo) == -1 and err().startswith("p_out overlaps b")
    assert _raw(osg, gpu, d, out[0], out[0], None, size, halo) == -1 and err().startswith("Gu overlaps Gv")
    assert _raw(osg, gpu, d, *out, size, halo, scheme=2) == -5 and "Coriolis scheme 2 is not built" in err()
    assert _raw(osg, gpu, d, *out, size, halo, mode=3) == -5 and "mode 3 is not built" in err()
    assert _raw(osg, gpu, d, *out, (20, 12, 5), (1, 1, 0)) == -5 and "Hz >= 1 needed (halo (1,1,0))" in err()
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)
    _assert_unchanged(d, h, "refusals")


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
@pytest.mark.parametrize("size,halo,tdt,scheme", [((48, 40, 6), (5, 5, 5), torch.float64, "enstrophy"), ((50, 40, 3), (4, 4, 4), torch.float32, "energy")],
                         ids=["48x40x6-h5-f64", "50x40x3-h4-f32-energy"])
def test_the_plan_equals_the_reference_and_replays_in_a_graph(osg, gpu, size, halo, tdt, scheme, immersed):
    """on a built grid with its own f, metrics and spacings: the plan's Gu, Gv and pressure are the reference's (masked on the immersed
    grid), it allocates nothing when called, and a captured graph replays the same bits; update_hydrostatic_pressure gives the same p"""
    from gpu_harness import _grid
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = _grid(osg, size, halo, tdt, immersed)
    g = getattr(grid, "underlying_grid", grid)
    gen = torch.Generator(device=gpu).manual_seed(5)
    u, Gu = osg.XFaceField(grid), osg.XFaceField(grid)
    v, Gv = osg.YFaceField(grid), osg.YFaceField(grid)
    b, p = osg.CenterField(grid), osg.CenterField(grid)
    for f in (u, v, b, Gu, Gv):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v, b])
    record = osg.HydrostaticSphericalCoriolis(scheme=osg.EnergyConserving() if scheme == "energy" else osg.EnstrophyConserving())
    f_ff = osg.coriolis_parameter(grid, record, tdt)
    assert f_ff is osg.coriolis_parameter(grid, record, tdt) and tuple(f_ff.shape) == tuple(u.data.shape[1:]) and f_ff.dtype == tdt
    start = [Gu.data.clone(), Gv.data.clone()]
    m = {k: g.arrays[k].cpu().numpy() for k in R.METRICS}
    dz = osg.z_all_face_spacings(grid, tdt).numpy().astype(m["dx_fc"].dtype)
    counts = getattr(grid, "column_counts", None)
    n = (None, None) if counts is None else (counts["fc"].cpu().numpy(), counts["cf"].cpu().numpy())
    host = lambda f: f.data.cpu().numpy()                          # noqa: E731
    with np.errstate(all="ignore"):
        want = R.tendencies(host(u), host(v), host(b), host(Gu), host(Gv), host(p), f_ff.cpu().numpy(), m, dz, size, halo,
                            ENERGY if scheme == "energy" else ENSTROPHY, ADD, *n, 0.0)
    plan = osg.hydrostatic_tendencies_plan(u, v, Gu, Gv, coriolis=record, b=b, pressure=p)
    assert plan() is plan
    eager = [host(Gu), host(Gv), host(p)]
    for name, got, w_ in zip(("Gu", "Gv", "p"), eager, want):
        _assert_parent(got, w_, name)
    _assert_parent(host(osg.update_hydrostatic_pressure(b)), want[2], "update_hydrostatic_pressure")
    for f, t in zip((Gu, Gv), start):
        f.data.copy_(t)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    plan()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before              # the plan allocates nothing when called
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            plan()
    torch.cuda.current_stream().wait_stream(side)
    for f, t in zip((Gu, Gv), start):
        f.data.copy_(t)
    p.data.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for name, f, w_ in zip(("Gu", "Gv"), (Gu, Gv), eager):
        _assert_parent(host(f), w_, ("replay", name))
    assert same_bits(host(p)[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], eager[2][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]) == 0


def test_the_example_steps_agree_eagerly_and_as_a_graph():
    """examples/hydrostatic_model_step.py asserts that its eager and replayed steps agree bit for bit"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "hydrostatic_model_step.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "agree bit for bit" in r.stdout and "True" in r.stdout.splitlines()[-1]
