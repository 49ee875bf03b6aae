"""GPU tests of the AB2 step of the velocities and tracers and of the barotropic forcing: tpg_ab2_step_velocities / tpg_ab2_step_fields through
the C ABI, and ab2_step_velocities / ab2_step_fields / the two plans through the package.  Compared BIT FOR BIT with tests/ab2_ref.py (numpy
in the fields' type: every operation of the rule is one correctly rounded IEEE operation and the column integral has one order, so the
reference is exact and there is no tolerance anywhere in this file); NaNs compare by NaN-ness; no case and no cell is left out of a
comparison: whole parents and planes, halo cells of written arrays against what they held, arrays not written against their input.

Shapes (size, halo, Hy2, type): the smallest at which each path can go wrong -- one level (the integral is one product); no halo at all; rows
off the 16-B grid with an odd Hx and Hy2 < Hy; more levels than twice the look-ahead and no multiple of it; the model halo 5 with
config 5's Hy2 = 31; Float32 with Nx = 2 mod 4 (8-B chunks); one shape with more work items than are resident; more levels than one segment
of the fields kernel; and one case past 2^31 elements.  dz_c is random in [0.5, 2], so a wrong k cannot hide."""

import numpy as np
import pytest
import torch

import ab2_ref as ref
import barotropic_ref
from ab2_ref import EULER, STORE, same_bits
from continuity_ref import w_and_divergence
from gpu_harness import _dev, _free_hbm  # noqa: F401
from immersed_ref import draw_columns, heights_of
from special_values import pool

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#         size            halo      Hy2  element type
TABLE = [((10, 10, 1), (4, 4, 4), 4, F64),         # one level: the integral is one product
         ((20, 12, 3), (0, 0, 0), 0, F64),         # no halo at all
         ((20, 12, 3), (0, 0, 0), 0, F32),
         ((20, 12, 3), (3, 2, 1), 1, F64),         # odd Hx, rows off the 16-B grid, Hy2 < Hy
         ((20, 12, 9), (4, 4, 4), 13, F64),        # more levels than twice the look-ahead, not a multiple of it
         ((48, 40, 6), (5, 5, 5), 31, F64),        # the model halo with config 5's Hy2
         ((48, 40, 6), (5, 5, 5), 31, F32),
         ((50, 40, 3), (4, 4, 4), 4, F32),         # Nx = 2 mod 4: 8-B chunks
         ((2304, 1283, 2), (4, 4, 4), 4, F64)]     # 1283 x 1152 chunks: more items than are resident
CROSS = [TABLE[3], TABLE[5], TABLE[6]]
SENTINEL = 12345.0
DT, CHI = 0.3, 0.1                                 # neither representable: converted once to the field type
FORMS = {"both": (True, True), "u": (True, False), "v": (False, True)}
KEYS = (("u", "Gu_n", "Gu_m", "GU"), ("v", "Gv_n", "Gv_m", "GV"))


def _id(case):
    size, halo, Hy2, dtype = case
    return "x".join(map(str, size)) + "-h" + "".join(map(str, halo)) + f"-{Hy2}" + ("-f64" if dtype == F64 else "-f32")


def _shapes(size, halo, Hy2):
    """(parent of the 3-D fields; 2-D plane)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy2, Nx + 2 * Hx)


_CASES = {}


def _case(case):
    """host arrays of a case, random in EVERY cell (halos included): u, v, their four tendencies, dz_c, the sentinel-filled planes GU, GV and
    the count planes (two drawn bottoms: land columns, open columns, everything between, one column above Nz and one negative count planted
    in each).  Computed once per case, shared by the tests, never modified (tests copy what they change)"""
    if case not in _CASES:
        size, halo, Hy2, dtype = case
        Nx, Ny, Nz = size
        parent, plane = _shapes(size, halo, Hy2)
        rng = np.random.default_rng([*size, *halo, Hy2, np.dtype(dtype).itemsize])
        h = {k: rng.uniform(-1, 1, parent).astype(dtype) for k in ("u", "v", "Gu_n", "Gv_n", "Gu_m", "Gv_m")}
        h["GU"], h["GV"] = np.full(plane, SENTINEL, dtype), np.full(plane, SENTINEL, dtype)
        h["dz_c"] = rng.uniform(0.5, 2, Nz).astype(dtype)
        for q, k in enumerate(("n_fc", "n_cf")):
            n = draw_columns(rng, Nx, Ny, Nz).astype(np.int32)
            n[Ny - 1, Nx - 1 - q], n[Ny - 2, Nx - 1 - q] = Nz + 3, -1 - q
            assert (n == 0).any() and (n == Nz).any() and (n > Nz).any() and (n < 0).any()
            h[k] = n
        for a in h.values():
            a.setflags(write=False)
        _CASES[case] = h
    return _CASES[case]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _velocities(osg, gpu, h, size, halo, Hy2, form="both", flags=STORE, integral=(True, True), counts=True, offset=0, null_gm=False,
                dt=DT, chi=CHI):
    """tpg_ab2_step_velocities on fresh device copies of h -> every array of the call on the host afterwards ({name: array}; a group the form
    leaves out, a plane `integral` leaves out and count planes not given are absent)"""
    has = FORMS[form]
    d = {}
    for q, (x, gn, gm, G) in enumerate(KEYS):
        if not has[q]:
            continue
        d[x], d[gn] = _dev(h[x], gpu, offset), _dev(h[gn], gpu, offset)
        if not null_gm:
            d[gm] = _dev(h[gm], gpu, offset)
        if integral[q]:
            d[G] = _dev(h[G], gpu, offset)
            if counts:
                d[("n_fc", "n_cf")[q]] = _dev(h[("n_fc", "n_cf")[q]], gpu, offset)
    if any(integral[q] and has[q] for q in range(2)):
        d["dz_c"] = _dev(h["dz_c"], gpu, offset)
    names = ("u", "v", "Gu_n", "Gv_n", "Gu_m", "Gv_m", "GU", "GV", "dz_c", "n_fc", "n_cf")
    osg._lib.check_timestep(osg._lib.timestep_lib().tpg_ab2_step_velocities(
        *(_ptr(d.get(k)) for k in names), dt, chi, flags, *size, *halo, Hy2, osg._lib.ft_of(d["u" if has[0] else "v"].dtype),
        osg._lib.current_stream_ptr(gpu)))
    return {k: t.cpu().numpy() for k, t in d.items()}


def _want_velocities(h, size, halo, Hy2, form="both", flags=STORE, integral=(True, True), counts=True, null_gm=False, dt=DT, chi=CHI):
    """the same dictionary from the reference: written arrays as the rule leaves them, the others as they were"""
    has = FORMS[form]
    out = {}
    for q, (x, gn, gm, G) in enumerate(KEYS):
        if not has[q]:
            continue
        n = h[("n_fc", "n_cf")[q]] if (integral[q] and counts) else None
        new, prev, plane = ref.ab2_step(h[x], h[gn], None if null_gm else h[gm], dt, chi, flags, size, halo, h[G] if integral[q] else None,
                                        h["dz_c"], Hy2, n)
        out[x], out[gn] = new, h[gn]
        if not null_gm:
            out[gm] = prev
        if integral[q]:
            out[G] = plane
            if counts:
                out[("n_fc", "n_cf")[q]] = n
    if any(integral[q] and has[q] for q in range(2)):
        out["dz_c"] = h["dz_c"]
    return out


def _assert_same(got, want, what):
    bad = same_bits(got, want) if got.dtype.kind == "f" else int((got != want).sum())
    assert bad == 0, (what, bad, "cells differ of", got.size)


def _assert_all(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in got:
        _assert_same(got[k], want[k], (what, k))


# ---- the C ABI: the velocities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_ab2_with_integral_and_store_is_bit_exact_on_whole_arrays(osg, gpu, case, offset):
    """random data in every cell, AB2 with the integral and the store, both fields, count planes given: u, v, Gu_m, Gv_m, GU, GV equal the
    reference's -- the interior the rule, every halo cell what it held (the planes: the sentinel) -- and Gu_n, Gv_n, dz_c, the count planes
    are as they were.  With every pointer on the 16-B grid and with every pointer one element past an allocation"""
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    want = _want_velocities(h, size, halo, Hy2)
    for x, gn, gm, G in KEYS:                                      # conditions on the reference alone
        inner = ref.cells_read(size, halo, Hy2)["field"]
        assert same_bits(want[x][~inner], h[x][~inner]) == 0 and (want[x][inner] != h[x][inner]).mean() > 0.9
        assert same_bits(want[gm][inner], h[gn][inner]) == 0 and same_bits(want[gm][~inner], h[gm][~inner]) == 0
        edge = np.ones(want[G].shape, bool)
        edge[Hy2:Hy2 + Ny, Hx:Hx + Nx] = False
        assert (want[G][edge] == SENTINEL).all() and not (want[G][~edge] == SENTINEL).any()
    _assert_all(_velocities(osg, gpu, h, size, halo, Hy2, offset=offset), want, "ab2 + integral + store")


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", CROSS, ids=_id)
def test_the_full_cross_of_forms_and_flags(osg, gpu, case, offset):
    """{both, u only, v only} x {AB2, EULER} x {store on, off} x {integral on, off} x {count planes given, NULL}.  Under EULER the previous
    tendencies are NaN in every cell: not read (no NaN arrives anywhere), with the store overwritten, without it left as they were.  Then
    what the cross leaves out: a NULL Gm under EULER alone, and the integral of one field only"""
    size, halo, Hy2, dtype = case
    h = _case(case)
    nan = dict(h, Gu_m=np.full(h["u"].shape, np.nan, dtype), Gv_m=np.full(h["u"].shape, np.nan, dtype))
    inner = ref.cells_read(size, halo, Hy2)["field"]
    for form in FORMS:
        for flags in (0, EULER, STORE, EULER | STORE):
            src = nan if flags & EULER else h
            for on in (True, False):
                for counts in ((True, False) if on else (False,)):  # the count planes mask the integral alone: without one they are not passed
                    kw = dict(form=form, flags=flags, integral=(on, on), counts=counts)
                    got = _velocities(osg, gpu, src, size, halo, Hy2, offset=offset, **kw)
                    _assert_all(got, _want_velocities(src, size, halo, Hy2, **kw), kw)
                    if flags & EULER:
                        for q, (x, gn, gm, G) in enumerate(KEYS):
                            if FORMS[form][q]:
                                assert not np.isnan(got[x]).any() and (not on or not np.isnan(got[G]).any())
                                assert np.isnan(got[gm][~inner]).all() and np.isnan(got[gm][inner]).all() != bool(flags & STORE)
    for form in FORMS:
        for on in (True, False):
            kw = dict(form=form, flags=EULER, integral=(on, on), null_gm=True)
            _assert_all(_velocities(osg, gpu, h, size, halo, Hy2, offset=offset, **kw), _want_velocities(h, size, halo, Hy2, **kw), kw)
    for integral in ((True, False), (False, True)):
        for flags in (STORE, EULER):
            kw = dict(flags=flags, integral=integral)
            _assert_all(_velocities(osg, gpu, h, size, halo, Hy2, offset=offset, **kw), _want_velocities(h, size, halo, Hy2, **kw), kw)
    # count planes given without a plane to integrate into are not read (the pointers are passed all the same)
    d = {k: _dev(h[k], gpu, offset) for k in ("u", "Gu_n", "Gu_m")}
    n = torch.full((size[1] * size[0] + offset,), 1 << 30, dtype=torch.int32, device=gpu)[offset:]
    osg._lib.check_timestep(osg._lib.timestep_lib().tpg_ab2_step_velocities(
        d["u"].data_ptr(), None, d["Gu_n"].data_ptr(), None, d["Gu_m"].data_ptr(), None, None, None, None, n.data_ptr(), None, DT, CHI, 0,
        *size, *halo, Hy2, osg._lib.ft_of(d["u"].dtype), osg._lib.current_stream_ptr(gpu)))
    _assert_same(d["u"].cpu().numpy(), _want_velocities(h, size, halo, Hy2, "u", 0, (False, False))["u"], "counts without a plane")


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", [TABLE[3], TABLE[7]], ids=_id)
def test_special_values_in_every_input(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max planted in 5 % of the cells of u, v and the four tendencies, one NaN and one +Inf explicitly in the
    interior, and one column whose g is -0 on every level (the integral is -0 only if the first term is the product itself): bit for bit
    numpy's, which computes the same IEEE operations.  AB2 and EULER, with and without count planes"""
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    rng = np.random.default_rng([7, *size, *halo])
    p = pool(dtype)
    planted = dict(h)
    for name in ("u", "v", "Gu_n", "Gv_n", "Gu_m", "Gv_m"):
        a = h[name].copy()
        where = rng.random(a.shape) < 0.05
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
        planted[name] = a
    for k in ("u", "Gu_n", "Gu_m"):                                # two open columns (counts 0) with finite data but for one cell each
        planted[k][Hz:Hz + Nz, Hy + 1:Hy + 3, Hx + 10:Hx + 12] = h[k][Hz:Hz + Nz, Hy + 1:Hy + 3, Hx + 10:Hx + 12]
    planted["Gu_n"][Hz, Hy + 1, Hx + 10], planted["Gu_n"][Hz + Nz - 1, Hy + 2, Hx + 11] = np.nan, np.inf
    planted["v"][Hz, Hy + 3, Hx + 1], planted["Gv_m"][Hz + Nz - 1, Hy + 4, Hx + 2] = np.nan, np.inf
    planted["Gu_n"][Hz:Hz + Nz, Hy, Hx + 9], planted["Gu_m"][Hz:Hz + Nz, Hy, Hx + 9] = -0.0, 0.0
    assert (h["n_fc"][0:3, 9:12] == 0).all()                       # open columns
    for flags in (STORE, EULER):
        for counts in (True, False):
            want = _want_velocities(planted, size, halo, Hy2, flags=flags, counts=counts)
            inner, gu = want["u"][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], want["GU"][Hy2:Hy2 + Ny, Hx:Hx + Nx]
            assert np.isfinite(inner).mean() >= 0.5 and np.isnan(inner).any() and np.isinf(inner).any()
            assert np.isfinite(gu).mean() >= 0.4 and np.isnan(gu).any() and np.isinf(gu).any() and gu[0, 9] == 0 and np.signbit(gu[0, 9])
            _assert_all(_velocities(osg, gpu, planted, size, halo, Hy2, flags=flags, counts=counts, offset=offset), want, ("special values", flags, counts))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_exact_integers_on_the_device(osg, gpu, dtype):
    """integer data, dt = 2, chi = 0.5 (c1 = 2, c2 = 1) and power-of-two dz_c through the C ABI: every result is the exact integer expression"""
    size, halo, Hy2 = (20, 12, 4), (2, 2, 1), 3
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = _shapes(size, halo, Hy2)
    rng = np.random.default_rng(9)
    h = {k: rng.integers(-9, 10, parent).astype(dtype) for k in ("u", "v", "Gu_n", "Gv_n", "Gu_m", "Gv_m")}
    h.update(GU=np.zeros(plane, dtype), GV=np.zeros(plane, dtype), dz_c=np.array([1, 2, 4, 1], dtype))
    got = _velocities(osg, gpu, h, size, halo, Hy2, flags=0, counts=False, dt=2.0, chi=0.5)
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx].astype(np.int64)
    for x, gn, gm, G in KEYS:
        g = 2 * cut(h[gn]) - cut(h[gm])
        assert np.array_equal(cut(got[x]), cut(h[x]) + 2 * g)
        assert np.array_equal(got[G][Hy2:Hy2 + Ny, Hx:Hx + Nx], (np.array([1, 2, 4, 1])[:, None, None] * g).sum(0).astype(dtype))


def test_latitude_bands_equal_the_global_field(osg, gpu):
    """40 x 24 x 3, halo 4, Hy2 = 6, global arrays; three bands of 8 rows cut as rows jstart - Hy .. jend + Hy of the parents (Hy2 for the
    planes) and the matching rows of the count planes: each band's outputs equal the matching rows of the global ones"""
    case = ((40, 24, 3), (4, 4, 4), 6, F64)
    size, halo, Hy2, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    want = _want_velocities(h, size, halo, Hy2)
    rows = 8
    for b in range(3):
        lo = b * rows                                              # 0-based padded row of the band's row jstart - Hy
        cut = {k: np.ascontiguousarray(h[k][:, lo:lo + rows + 2 * Hy, :]) for k in ("u", "v", "Gu_n", "Gv_n", "Gu_m", "Gv_m")}
        cut.update({k: np.ascontiguousarray(h[k][lo:lo + rows + 2 * Hy2, :]) for k in ("GU", "GV")})
        cut.update({k: np.ascontiguousarray(h[k][lo:lo + rows]) for k in ("n_fc", "n_cf")})
        cut["dz_c"] = h["dz_c"]
        bsize = (Nx, rows, Nz)
        got = _velocities(osg, gpu, cut, bsize, halo, Hy2)
        _assert_all(got, _want_velocities(cut, bsize, halo, Hy2), ("band", b))
        for k in ("u", "v", "Gu_m", "Gv_m"):
            _assert_same(got[k][Hz:Hz + Nz, Hy:Hy + rows, Hx:Hx + Nx], want[k][Hz:Hz + Nz, Hy + lo:Hy + lo + rows, Hx:Hx + Nx], ("band rows", b, k))
        for k in ("GU", "GV"):
            _assert_same(got[k][Hy2:Hy2 + rows, Hx:Hx + Nx], want[k][Hy2 + lo:Hy2 + lo + rows, Hx:Hx + Nx], ("band rows", b, k))


# ---- the C ABI: the fields -----------------------------------------------------------------------------------------------------------------
FIELD_CASES = [((20, 12, 3), (3, 2, 1), F64), ((50, 40, 3), (4, 4, 4), F32), ((20, 12, 77), (1, 1, 1), F64)]     # the last: many segments of levels, the last one short
_FIELDS = {}


def _field_case(case):
    if case not in _FIELDS:
        size, halo, dtype = case
        parent, _ = _shapes(size, halo, 0)
        rng = np.random.default_rng([5, *size, *halo, np.dtype(dtype).itemsize])
        h = [tuple(rng.uniform(-1, 1, parent).astype(dtype) for _ in range(3)) for _ in range(16)]
        for t in h:
            for a in t:
                a.setflags(write=False)
        _FIELDS[case] = h
    return _FIELDS[case]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("case", FIELD_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-h" + "".join(map(str, c[1])) + ("-f64" if c[2] == F64 else "-f32"))
def test_fields_call_with_1_3_and_16_fields(osg, gpu, case, n, offset):
    """n fields in ONE call, {AB2, EULER} x {store on, off}: every field, and every previous tendency under the store, equals the reference's
    whole parent; Gn, and Gm without the store, are as they were.  Under EULER Gm is NaN in every cell; under EULER alone also NULL"""
    size, halo, dtype = case
    h = _field_case(case)[:n]
    lib = osg._lib.timestep_lib()
    inner = ref.cells_read(size, halo)["field"]
    for flags in (0, EULER, STORE, EULER | STORE):
        for null_gm in ((False, True) if flags == EULER else (False,)):
            gm_host = [np.full(t[2].shape, np.nan, dtype) if flags & EULER else t[2] for t in h]
            x, gn = [_dev(t[0], gpu, offset) for t in h], [_dev(t[1], gpu, offset) for t in h]
            gm = None if null_gm else [_dev(a, gpu, offset) for a in gm_host]
            osg._lib.check_timestep(lib.tpg_ab2_step_fields(osg._lib.ptr_table(x), osg._lib.ptr_table(gn), None if null_gm else osg._lib.ptr_table(gm),
                                                            n, DT, CHI, flags, *size, *halo, osg._lib.ft_of(x[0].dtype), osg._lib.current_stream_ptr(gpu)))
            for f in range(n):
                new, prev, _ = ref.ab2_step(h[f][0], h[f][1], None if null_gm else gm_host[f], DT, CHI, flags, size, halo)
                _assert_same(x[f].cpu().numpy(), new, ("field", f, flags))
                _assert_same(gn[f].cpu().numpy(), h[f][1], ("Gn", f, flags))
                if not null_gm:
                    _assert_same(gm[f].cpu().numpy(), prev, ("Gm", f, flags))
                assert not np.isnan(new[inner]).any() and (new[inner] != h[f][0][inner]).mean() > 0.9


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
def _np_type(tdt):
    return F64 if tdt == torch.float64 else F32


def _filled(osg, like, interior, base):
    """the parent fill_halo_regions gives a field at `like`'s location and grid that held `base` (a parent) and got that interior"""
    f = osg.Field(like.loc, like.grid)
    f.data.copy_(torch.from_numpy(np.ascontiguousarray(base)).reshape(f.data.shape))
    f.interior().copy_(torch.from_numpy(np.ascontiguousarray(interior)).reshape(f.interior().shape))
    osg.fill_halo_regions([f])
    return f.data.cpu().numpy()


def _immersed(osg, size, halo, tdt, seed=19):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    base = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
    zc = base.z_centers[Hz:Hz + Nz].cpu().numpy()
    rng = np.random.default_rng(seed)
    ibg = osg.ImmersedBoundaryGrid(base, osg.GridFittedBottom(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)))
    nfc, ncf = (ibg.column_counts[k].cpu().numpy() for k in ("fc", "cf"))
    assert (nfc >= Nz).any() and (nfc == 0).any() and ((nfc > 0) & (nfc < Nz)).any()
    return base, ibg, nfc, ncf


def _velocity_fields(osg, gpu, grid, seed=3):
    gen = torch.Generator(device=gpu).manual_seed(seed)
    out = [osg.XFaceField(grid), osg.YFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid)]
    for f in out:
        f.data.uniform_(-1, 1, generator=gen)
    return out                                                     # u, v, Gu, Gv, Gu_prev, Gv_prev


def _host(fields):
    return [None if f is None else f.data.cpu().numpy() for f in fields]


def _ref_package_step(osg, grid, host, planes, dt, chi, flags, counts, fill, fields):
    """the whole arrays (u, v, Gu_prev, Gv_prev, GU, GV) the package call leaves, from host copies: the rule with the grid's own
    z_center_spacings, then (with `fill`) the fill of u and v"""
    u, v, Gu, Gv, Gup, Gvp = host
    g = getattr(grid, "underlying_grid", grid)
    size, halo = (g.Nx, g.Ny, g.Nz), (g.Hx, g.Hy, g.Hz)
    dz = osg.z_center_spacings(grid, fields[0].data.dtype).numpy().astype(u.dtype)
    out = []
    for x, gn, gm, G, n, f in ((u, Gu, Gup, planes[0], counts[0], fields[0]), (v, Gv, Gvp, planes[1], counts[1], fields[1])):
        Hy2 = 0 if G is None else (G.shape[-2] - g.Ny) // 2
        new, prev, plane = ref.ab2_step(x, gn, gm, dt, chi, flags, size, halo, None if G is None else G[0], dz, Hy2, n)
        if fill:
            new = _filled(osg, f, new[halo[2]:halo[2] + g.Nz, halo[1]:halo[1] + g.Ny, halo[0]:halo[0] + g.Nx], x)
        out.append((new, prev, None if plane is None else plane[None]))
    return [out[0][0], out[1][0], out[0][1], out[1][1], out[0][2], out[1][2]]


@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)], ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_velocity_step_through_the_package(osg, gpu, size, halo, tdt):
    """u, v on an ImmersedBoundaryGrid, GU, GV the planes of a 12-sub-step SplitExplicitFreeSurface on with_halo((Hx, 13, Hz), grid): the
    count planes mask the integral; with fill_halos the parents of u, v are what fill_halo_regions gives; mask_immersed=False integrates
    every level; a pair alone; euler; the planes on the fields' own grid; with_dt"""
    base, ibg, nfc, ncf = _immersed(osg, size, halo, tdt)
    fs = osg.SplitExplicitFreeSurface(ibg, substeps=12)
    assert fs.GU.Hy == 13 and fs.extended_grid is not base
    gen = torch.Generator(device=gpu).manual_seed(11)

    def fresh():
        fields = _velocity_fields(osg, gpu, ibg)
        for f in (fs.GU, fs.GV):
            f.data.uniform_(-1, 1, generator=gen)
        return fields, _host(fields), _host([fs.GU, fs.GV])

    def check(fields, planes, want, what):
        for f, w, k in zip((*fields[:2], *fields[4:], *planes), want, ("u", "v", "Gu_prev", "Gv_prev", "GU", "GV")):
            assert (f is None) == (w is None), (what, k)
            if f is not None:
                _assert_same(f.data.cpu().numpy(), w, (what, k))

    fields, host, planes = fresh()
    got = osg.ab2_step_velocities(*fields, DT, chi=CHI, GU=fs.GU, GV=fs.GV, fill_halos=True)
    assert got[0] is fields[0] and got[1] is fields[1]
    want = _ref_package_step(osg, ibg, host, planes, DT, CHI, STORE, (nfc, ncf), True, fields)
    check(fields, (fs.GU, fs.GV), want, "immersed, filled")
    plain = _ref_package_step(osg, ibg, host, planes, DT, CHI, STORE, (None, None), True, fields)
    assert same_bits(want[4], plain[4]) > 0 and same_bits(want[0], plain[0]) == 0     # the count planes matter, to the integral alone
    for f, g0 in zip(fields[2:4], host[2:4]):
        _assert_same(f.data.cpu().numpy(), g0, "Gn as it was")
    # no mask, no fill, chi left to its default, no store
    fields, host, planes = fresh()
    plan = osg.ab2_velocity_step_plan(*fields, DT, GU=fs.GU, GV=fs.GV, mask_immersed=False, store_tendencies=False)
    assert plan() is plan and plan.u is fields[0] and plan.GV is fs.GV
    check(fields, (fs.GU, fs.GV), _ref_package_step(osg, ibg, host, planes, DT, 0.1, 0, (None, None), False, fields), "plain")
    # with_dt: the same tensors, the new step
    host, planes = _host(fields), _host([fs.GU, fs.GV])
    again = plan.with_dt(0.7)
    assert again() is again
    check(fields, (fs.GU, fs.GV), _ref_package_step(osg, ibg, host, planes, 0.7, 0.1, 0, (None, None), False, fields), "with_dt")
    # euler with chi = -0.5 and no previous tendency at all; u alone with its plane
    fields, host, planes = fresh()
    osg.ab2_step_velocities(fields[0], None, fields[2], None, None, None, DT, chi=-0.5, GU=fs.GU, euler=True, store_tendencies=False)
    want = _ref_package_step(osg, ibg, host, planes, DT, -0.5, EULER, (nfc, None), False, fields)
    _assert_same(fields[0].data.cpu().numpy(), want[0], "euler u")
    _assert_same(fs.GU.data.cpu().numpy(), want[4], "euler GU")
    dz = osg.z_center_spacings(ibg, tdt).numpy().astype(_np_type(tdt))
    for f, h0 in zip((fields[1], fields[4], fs.GV), (host[1], host[4], planes[1])):
        _assert_same(f.data.cpu().numpy(), h0, "left alone")
    assert dz.shape == (size[2],)
    # v alone, euler with the store, the plane on the fields' own grid (Hy2 = Hy)
    fields, host, _ = fresh()
    GV = osg.Field(fs.GV.loc, ibg)
    GV.data.uniform_(-1, 1, generator=gen)
    planes = [None, GV.data.cpu().numpy()]
    osg.ab2_step_velocities(None, fields[1], None, fields[3], None, fields[5], DT, chi=CHI, GV=GV, euler=True)
    want = _ref_package_step(osg, ibg, host, planes, DT, CHI, EULER | STORE, (None, ncf), False, fields)
    for f, w, k in ((fields[1], want[1], "v"), (fields[5], want[3], "Gv_prev"), (GV, want[5], "GV"), (fields[0], host[0], "u")):
        _assert_same(f.data.cpu().numpy(), w, ("v alone", k))
    # without planes: the step alone
    fields, host, _ = fresh()
    osg.ab2_step_velocities(*fields, DT, chi=CHI)
    check(fields, (None, None), _ref_package_step(osg, ibg, host, [None, None], DT, CHI, STORE, (None, None), False, fields), "no integral")


def test_fields_step_through_the_package(osg, gpu):
    """two tracers, then 18 (two calls), on a built grid: ab2_step_fields, the plan, with_dt, fill_halos"""
    size, halo = (48, 40, 6), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = osg.TripolarGrid(osg.GPU(0), torch.float32, size=size, halo=halo, z=(-1, 0))
    gen = torch.Generator(device=gpu).manual_seed(23)

    def fresh(n):
        sets = [[osg.CenterField(grid) for _ in range(n)] for _ in range(3)]
        for fs in sets:
            for f in fs:
                f.data.uniform_(-1, 1, generator=gen)
        return sets, [_host(fs) for fs in sets]

    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    (c, Gn, Gm), host = fresh(2)
    assert osg.ab2_step_fields(c, Gn, Gm, DT, chi=CHI, fill_halos=True) == c
    for q in range(2):
        new, prev, _ = ref.ab2_step(host[0][q], host[1][q], host[2][q], DT, CHI, STORE, size, halo)
        _assert_same(c[q].data.cpu().numpy(), _filled(osg, c[q], cut(new), host[0][q]), ("tracer", q))
        _assert_same(Gm[q].data.cpu().numpy(), prev, ("Gm", q))
        _assert_same(Gn[q].data.cpu().numpy(), host[1][q], ("Gn", q))
    (c, Gn, Gm), host = fresh(18)
    plan = osg.ab2_step_plan(c, Gn, None, DT, euler=True, store_tendencies=False)
    assert plan() is plan and len(plan._before) == 1
    for q in range(18):
        new, _, _ = ref.ab2_step(host[0][q], host[1][q], None, DT, 0.1, EULER, size, halo)
        _assert_same(c[q].data.cpu().numpy(), new, ("18 tracers", q))
    host[0] = _host(c)
    assert plan.with_dt(1.5)() is not plan
    for q in range(18):
        new, _, _ = ref.ab2_step(host[0][q], host[1][q], None, 1.5, 0.1, EULER, size, halo)
        _assert_same(c[q].data.cpu().numpy(), new, ("18 tracers, with_dt", q))


def test_plans_replay_in_a_graph_and_allocate_nothing(osg, gpu):
    """both plans captured in ONE graph (a single chain, no parallel branches) and replayed twice equal two eager calls; calling them
    allocates nothing"""
    size, halo = (48, 40, 6), (4, 4, 4)
    base, ibg, nfc, ncf = _immersed(osg, size, halo, torch.float64)
    fs = osg.SplitExplicitFreeSurface(ibg, substeps=12)
    fields = _velocity_fields(osg, gpu, ibg)
    tracers = [[osg.CenterField(ibg) for _ in range(2)] for _ in range(3)]
    gen = torch.Generator(device=gpu).manual_seed(29)
    for f in (*tracers[0], *tracers[1], *tracers[2]):
        f.data.uniform_(-1, 1, generator=gen)
    vel = osg.ab2_velocity_step_plan(*fields, DT, chi=CHI, GU=fs.GU, GV=fs.GV, fill_halos=True)
    trc = osg.ab2_step_plan(*tracers, DT, chi=CHI, fill_halos=True)
    everything = [*fields, fs.GU, fs.GV, *tracers[0], *tracers[1], *tracers[2]]
    start = [f.data.clone() for f in everything]
    vel(); trc()                                                   # eager warm-up (first-call work outside the capture)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    vel(); trc()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before
    eager = [f.data.clone() for f in everything]                   # two eager calls from `start`
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            vel()
            trc()
    torch.cuda.current_stream().wait_stream(side)
    for f, t in zip(everything, start):
        f.data.copy_(t)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for f, t in zip(everything, eager):
        _assert_same(f.data.cpu().numpy(), t.cpu().numpy(), ("replayed twice", f.name))
    assert same_bits(everything[0].data.cpu().numpy(), start[0].cpu().numpy()) > 0


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_the_whole_step_against_the_references_chained(osg, gpu, tdt):
    """(48, 40, 6), halo 5, 12 sub-steps, an immersed grid: tendencies -> ab2_velocity_step_plan writing the free surface's GU, GV ->
    barotropic_mode_plan -> split_explicit_subcycle_plan -> barotropic_correction_plan -> continuity_plan, every output (u, v, the forcing,
    eta, U, V, the twins, the averages, w) bit for bit the composition of ab2_ref, barotropic_ref, free_surface_ref, continuity_ref and the
    fill's.  Each stage's reference starts from the previous stage's outputs, which were just held equal to THEIR reference: the composition
    by induction.  This is the test that GU, GV land where the sub-step reads them"""
    from test_gpu_free_surface import _assert_free_surface, _reference_subcycle
    size, halo, substeps, dtau = (48, 40, 6), (5, 5, 5), 12, 0.05
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    T = _np_type(tdt)
    base, ibg, nfc, ncf = _immersed(osg, size, halo, tdt)
    ncc = ibg.column_counts["cc"].cpu().numpy()
    fs = osg.SplitExplicitFreeSurface(ibg, substeps=substeps)
    ext = fs.extended_grid
    assert ext.Hy == 13
    gen = torch.Generator(device=gpu).manual_seed(4)
    for f in (*fs.state, fs.GU, fs.GV, *fs.twins, *fs.averages):
        f.data.uniform_(-0.01, 0.01, generator=gen)
    osg.fill_halo_regions(list(fs.state))
    fields = _velocity_fields(osg, gpu, ibg)
    for f in fields[2:]:
        f.data.mul_(0.01)                                          # tendencies that leave the sub-cycle finite
    u, v = fields[:2]
    w = osg.ZFaceField(ibg)
    Ub, Vb = osg.Field(fs.U.loc, ext, name="Ubar"), osg.Field(fs.V.loc, ext, name="Vbar")
    step = osg.ab2_velocity_step_plan(*fields, DT, chi=CHI, GU=fs.GU, GV=fs.GV, fill_halos=True)
    mode = osg.barotropic_mode_plan(u, v, Ub, Vb)
    subcycle = osg.split_explicit_subcycle_plan(fs, dtau)
    correction = osg.barotropic_correction_plan(u, v, fs.U, fs.V, Ub, Vb)
    continuity = osg.continuity_plan(u, v, w)
    # the head: the AB2 step and the forcing
    host, planes = _host(fields), _host([fs.GU, fs.GV])
    step()
    want = _ref_package_step(osg, ibg, host, planes, DT, CHI, STORE, (nfc, ncf), True, fields)
    for f, wnt, k in zip((u, v, fields[4], fields[5], fs.GU, fs.GV), want, ("u", "v", "Gu_prev", "Gv_prev", "GU", "GV")):
        _assert_same(f.data.cpu().numpy(), wnt, ("chain: head", k))
    inner_GU = want[4][0, ext.Hy:ext.Hy + Ny, Hx:Hx + Nx]
    assert (inner_GU != 0).mean() > 0.5 and same_bits(inner_GU, planes[0][0, ext.Hy:ext.Hy + Ny, Hx:Hx + Nx]) > 0.9 * inner_GU.size
    # the mode of the stepped velocities
    dz = osg.z_center_spacings(base, tdt).numpy().astype(T)
    held = _host([Ub, Vb])
    mode()
    for f, hf, b in ((Ub, want[0], held[0]), (Vb, want[1], held[1])):
        _assert_same(f.data.cpu().numpy(), _filled(osg, f, barotropic_ref.interior_mode(hf, dz, size, halo), b), ("chain: mode", f.name))
    fs.U.data.copy_(Ub.data)
    fs.V.data.copy_(Vb.data)
    # the sub-cycle, forced by GU, GV
    sub = _reference_subcycle(osg, fs, dtau, nfc, ncf)
    for f in (fs.GU, fs.GV):
        f.data.neg_()
    other = _reference_subcycle(osg, fs, dtau, nfc, ncf)
    for f in (fs.GU, fs.GV):
        f.data.neg_()
    assert same_bits(sub[0][1], other[0][1]) > 0                    # the forcing matters
    subcycle()
    _assert_free_surface(fs, sub, "chain: sub-cycle")
    # the correction and w
    correction()
    depth = osg.column_depth_table(base, tdt).numpy().astype(T)
    filled = []
    for f, hf, t, tb, n in ((u, want[0], sub[0][1], Ub, nfc), (v, want[1], sub[0][2], Vb, ncf)):
        c = barotropic_ref.interior_correction(hf, t[0], tb.data[0].cpu().numpy(), depth, size, halo, ext.Hy, n, 0.0)
        filled.append(_filled(osg, f, c, hf))
        _assert_same(f.data.cpu().numpy(), filled[-1], ("chain: corrected", f.name))
    w0 = w.data.cpu().numpy()
    continuity()
    metrics = [base.arrays[k].cpu().numpy() for k in ("dy_fc", "dx_cf", "az_cc")]
    want_w, _ = w_and_divergence(filled[0], filled[1], w0, None, *metrics, dz, size, halo, ncc, 0.0)
    _assert_same(w.data.cpu().numpy(), _filled(osg, w, want_w[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx], w0), "chain: w")


# ---- past 2^31 elements --------------------------------------------------------------------------------------------------------------------
def test_float32_past_2g_elements(osg, gpu):
    """8640 x 4320 x 64, halo 5, Float32, u only with the integral and the store: 2.8e9 elements in a parent, so the element offsets of the
    upper levels need 64 bits.  The data is drawn on the device; the reference is built on the device level by level with torch's separate
    elementwise operations (each one correctly rounded IEEE operation, none fused) BEFORE the call, and compared on integer views: every
    level of u and of Gu_m in full, GU in full, the halo slabs of u.  Peak memory under half the card"""
    from test_gpu_past_2g import _budget, _ints
    size, halo, Hy2 = (8640, 4320, 64), (5, 5, 5), 5
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = _shapes(size, halo, Hy2)
    assert parent[0] * parent[1] * parent[2] > 1 << 31
    inner2 = (slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    with _budget(gpu, "ab2 velocities"):
        gen = torch.Generator(device=gpu).manual_seed(5)
        u = torch.empty(parent, dtype=torch.float32, device=gpu).uniform_(-1, 1, generator=gen)
        gn = torch.empty(parent, dtype=torch.float32, device=gpu).uniform_(-1, 1, generator=gen)
        gm = torch.empty(parent, dtype=torch.float32, device=gpu).uniform_(-1, 1, generator=gen)
        dz = torch.empty(Nz, dtype=torch.float32, device=gpu).uniform_(0.5, 2, generator=gen)
        n = torch.randint(-1, Nz + 2, (Ny, Nx), dtype=torch.int32, device=gpu, generator=gen)
        GU = torch.full(plane, SENTINEL, dtype=torch.float32, device=gpu)
        c1, c2, dt = (float(c) for c in ref.constants(DT, CHI, F32))
        hdz = [float(d) for d in dz.cpu().numpy()]
        m = n.clamp(0, Nz)
        want = u.clone()                                           # halo cells: as they were
        acc = None
        for k in range(Nz):
            g = gn[Hz + k][inner2] * c1 - gm[Hz + k][inner2] * c2
            want[Hz + k][inner2] = u[Hz + k][inner2] + g * dt
            gh = torch.where(k + 1 <= m, torch.zeros_like(g), g)
            acc = gh * hdz[k] if k == 0 else acc + gh * hdz[k]
        del g, gh
        want_GU = torch.full(plane, SENTINEL, dtype=torch.float32, device=gpu)
        want_GU[Hy2:Hy2 + Ny, Hx:Hx + Nx] = acc
        edge = torch.ones(parent[1:], dtype=torch.bool, device=gpu)
        edge[inner2] = False
        held = gm[Hz + Nz // 2][edge].clone()                      # a halo ring of Gu_m
        osg._lib.check_timestep(osg._lib.timestep_lib().tpg_ab2_step_velocities(
            u.data_ptr(), None, gn.data_ptr(), None, gm.data_ptr(), None, GU.data_ptr(), None, dz.data_ptr(), n.data_ptr(), None, DT, CHI, STORE,
            *size, *halo, Hy2, osg._lib.TPG_F32, osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        assert bool((_ints(GU) == _ints(want_GU)).all()) and bool(torch.isfinite(acc).all()) and float((acc != 0).float().mean()) > 0.9
        for k in range(parent[0]):                                 # every level and both halo slabs, level by level (no second full-size mask)
            assert bool((_ints(u[k]) == _ints(want[k])).all()), k
        for k in range(Nz):
            assert bool((_ints(gm[Hz + k][inner2]) == _ints(gn[Hz + k][inner2])).all()), k
        assert bool((_ints(gm[Hz + Nz // 2][edge]) == _ints(held)).all())
        assert not bool((_ints(u[Hz + Nz - 1][inner2]) == _ints(gn[Hz + Nz - 1][inner2])).all())
