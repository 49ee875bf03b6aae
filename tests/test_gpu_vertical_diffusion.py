"""GPU tests of the vertically implicit diffusion step (tpg_vertical_implicit_diffusion, libtripolar_hip_vertical_diffusion.so): bit for bit
against tests/vertical_diffusion_ref.py on WHOLE parents -- no tolerance anywhere.  NaN sits in every cell the header says is not read: the
halos of the fields, the kappa planes of the faces 1 and Nz + 1, the kappa halos, dz_f[1] and dz_f[Nz+1], and all of scratch (whose halo must
still hold it afterwards); the halos and kappa must come back unchanged.

The shapes are the smallest at which each path can go wrong (the table of CASES); every kappa form x both paths x masked and unmasked meets
the smallest shape and the nine-level shape, the other shapes take the combinations in rotation."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import special_values as sv
import vertical_diffusion_ref as R
from gpu_harness import F32, F64, TWO31, _assert_parent, _budget, _dev, _free_hbm, _id  # noqa: F401
from immersed_ref import draw_columns
from vorticity_ref import same_bits

pytestmark = pytest.mark.gpu

AUTO, ON_CHIP, STREAMED = 0, 1, 2
FORMS = {"constant": R.CONSTANT, "profile": R.PROFILE, "field": R.FIELD}
PATHS = {"on_chip": ON_CHIP, "streamed": STREAMED}
DT = 0.7
KAPPA = 0.37

SMALLEST = ((2, 1, 1), (1, 1, 1), F64)
NINE = ((20, 10, 9), (4, 4, 4), F64)                               # more levels than twice the look-ahead (4), and no multiple of it
CASES = [SMALLEST,
         ((10, 10, 2), (4, 4, 4), F64),                            # one face: one elimination, one back step
         ((20, 12, 3), (1, 1, 1), F64), ((20, 12, 3), (1, 1, 1), F32),   # the first row with two neighbours
         ((20, 12, 3), (3, 2, 1), F64),                            # odd Hx: the element-aligned chunks
         NINE,
         ((24, 11, 5), (4, 4, 4), F32),                            # odd Ny
         ((48, 40, 6), (5, 5, 5), F64), ((48, 40, 6), (5, 5, 5), F32),   # the model halo
         ((50, 40, 3), (4, 4, 4), F32)]                            # 8-B chunks
MANY = ((2304, 1283, 2), (4, 4, 4), F64)                           # more items than are resident


def _combos():
    every = list(itertools.product(FORMS, PATHS, (False, True)))
    out = [(case, *c) for case in (SMALLEST, NINE) for c in every]
    rest = [c for c in CASES if c not in (SMALLEST, NINE)]
    out += [(case, *every[(5 * q + r) % len(every)]) for q, case in enumerate(rest) for r in (0, 7)]
    return out


def _combo_id(c):
    case, form, path, masked = c
    return f"{_id(case)}-{form}-{path}-{'masked' if masked else 'open'}"


def _counts(size, seed=0):
    """a drawn bottom with negative counts, 0, Nz - 1 (one wet cell), Nz and beyond planted"""
    Nx, Ny, Nz = size
    n = draw_columns(np.random.default_rng([31 + seed, *size]), Nx, Ny, Nz).astype(np.int32)
    flat = n.reshape(-1)
    for q, v in enumerate((-2, 0, Nz - 1, Nz, Nz + 3)):
        flat[(q * 7) % flat.size if flat.size > 5 else q % flat.size] = v
    if flat.size <= 5:                                             # two columns: a masked one and one with the top cell wet
        flat[0], flat[-1] = Nz + 3, Nz - 1
    return n


_DRAWN = {}


def _problem(case, form, nfields=1):
    """host arrays of a case, drawn once and never modified: `fields` (interior in [-1, 1], NaN halos), `kappa` in the form, dz_c and dz_f
    in [0.5, 2] (NaN at the two closed faces)"""
    key = (case, form, nfields)
    if key not in _DRAWN:
        size, halo, dtype = case
        (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
        rng = np.random.default_rng([*size, *halo, np.dtype(dtype).itemsize, FORMS[form]])
        shape = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
        inner = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
        fields = []
        for _ in range(nfields):
            f = np.full(shape, np.nan, dtype)
            f[inner] = rng.uniform(-1, 1, (Nz, Ny, Nx))
            fields.append(f)
        dz_c = rng.uniform(0.5, 2, Nz).astype(dtype)
        dz_f = rng.uniform(0.5, 2, Nz + 1).astype(dtype)
        dz_f[0] = dz_f[Nz] = np.nan
        if form == "constant":
            kappa = KAPPA
        elif form == "profile":
            kappa = rng.uniform(0, 2, Nz + 1).astype(dtype)
            kappa[0] = kappa[Nz] = np.nan
        else:
            kappa = np.full(shape, np.nan, dtype)
            kappa[Hz + 1:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = rng.uniform(0, 2, (max(Nz - 1, 0), Ny, Nx))
        for a in (*fields, dz_c, dz_f, *([kappa] if form != "constant" else [])):
            a.setflags(write=False)
        _DRAWN[key] = dict(fields=fields, kappa=kappa, dz_c=dz_c, dz_f=dz_f)
    return _DRAWN[key]


_WANT = {}


def _want(case, form, masked, nfields=1, dt=DT):
    key = (case, form, masked, nfields, dt)
    if key not in _WANT:
        size, halo, _ = case
        h = _problem(case, form, nfields)
        _WANT[key] = R.reference(h["fields"], h["kappa"], FORMS[form], h["dz_c"], h["dz_f"], dt, size, halo, _counts(size) if masked else None, 0.0)
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def _solve(osg, gpu, fields, kappa, form, dz_c, dz_f, counts, scratch, path, size, halo, dt=DT, mask_value=0.0, kappa_value=0.0):
    """the status of the entry point on device tensors (kappa, counts, scratch: a tensor or None)"""
    L = osg._lib
    ptr = lambda t: None if t is None else t.data_ptr()           # noqa: E731
    return L.vertical_diffusion_lib().tpg_vertical_implicit_diffusion(
        L.ptr_table(fields), len(fields), ptr(kappa), kappa_value, form, ptr(dz_c), ptr(dz_f), ptr(counts), mask_value, dt, ptr(scratch), path,
        *size, *halo, L.ft_of(fields[0].dtype), L.current_stream_ptr(gpu))


def _run(osg, gpu, case, form, path, masked, nfields=1, which=None, offset=0, dt=DT):
    """the call on device copies of the case's problem (the fields `which`: indices; None: all) -> the whole parents on the host.  Asserts
    that kappa and the halo of scratch are untouched"""
    size, halo, dtype = case
    h = _problem(case, form, nfields)
    hosts = h["fields"] if which is None else [h["fields"][q] for q in which]
    fields = [_dev(f, gpu, offset) for f in hosts]
    kappa = None if form == "constant" else _dev(h["kappa"], gpu, offset)
    counts = _dev(_counts(size), gpu) if masked else None
    scratch = _dev(np.full(hosts[0].shape, np.nan, dtype), gpu, offset)
    status = _solve(osg, gpu, fields, kappa, FORMS[form], _dev(h["dz_c"], gpu, offset), _dev(h["dz_f"], gpu, offset), counts,
                    scratch if path != ON_CHIP else None, path, size, halo, dt, kappa_value=KAPPA if form == "constant" else 0.0)
    osg._lib.check_vertical_diffusion(status)
    torch.cuda.synchronize()
    if kappa is not None:
        _assert_parent(kappa.cpu().numpy(), h["kappa"], "kappa unchanged")
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    s = scratch.cpu().numpy()
    s[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = np.nan
    assert np.isnan(s).all(), "a halo cell of scratch was written"
    return [f.cpu().numpy() for f in fields]


# ---- the table: every shape, the forms, paths and the mask crossed sparsely -------------------------------------------------------------------------
@pytest.mark.parametrize("combo", _combos(), ids=_combo_id)
def test_whole_parents_are_the_reference_bit_for_bit(osg, gpu, combo):
    case, form, path, masked = combo
    if masked:
        n, Nz = _counts(case[0]), case[0][2]
        assert (n < 0).any() or n.size <= 5
        assert (n >= Nz).any() and ((n == Nz - 1).any() or Nz == 1)
    got = _run(osg, gpu, case, form, PATHS[path], masked)
    _assert_parent(got[0], _want(case, form, masked)[0], combo)


def test_every_pointer_one_element_off_the_16_byte_grid(osg, gpu):
    case = ((20, 12, 3), (3, 2, 1), F64)
    for form, path, masked in (("field", STREAMED, True), ("profile", ON_CHIP, False)):
        got = _run(osg, gpu, case, form, path, masked, offset=1)
        _assert_parent(got[0], _want(case, form, masked)[0], (form, path, masked))


@pytest.mark.parametrize("path", PATHS)
def test_more_items_than_are_resident(osg, gpu, path):
    got = _run(osg, gpu, MANY, "field", PATHS[path], True)
    _assert_parent(got[0], _want(MANY, "field", True)[0], path)


@pytest.mark.parametrize("case", [((20, 12, 3), (1, 1, 1), F64), ((48, 40, 6), (5, 5, 5), F32)], ids=_id)
@pytest.mark.parametrize("path", PATHS)
def test_n_fields_in_one_call_equal_their_one_field_calls(osg, gpu, case, path):
    """n = 1, 2, 3 and 16: one matrix, n right-hand sides.  Each field's bits are those of its one-field call and the reference's"""
    want = _want(case, "field", True, nfields=16)
    alone = [_run(osg, gpu, case, "field", PATHS[path], True, nfields=16, which=[q])[0] for q in range(16)]
    for q in range(16):
        _assert_parent(alone[q], want[q], ("alone", q))
    for n in (2, 3, 16):
        together = _run(osg, gpu, case, "field", PATHS[path], True, nfields=16, which=list(range(16 - n, 16)))
        for q, got in zip(range(16 - n, 16), together):
            _assert_parent(got, alone[q], (n, q))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_on_chip_and_streamed_give_identical_bits(osg, gpu, dtype):
    case = ((48, 40, 6), (5, 5, 5), dtype)
    for form in FORMS:
        a = _run(osg, gpu, case, form, ON_CHIP, True, nfields=3)
        b = _run(osg, gpu, case, form, STREAMED, True, nfields=3)
        c = _run(osg, gpu, case, form, AUTO, True, nfields=3)
        for x, y, z in zip(a, b, c):
            _assert_parent(x, y, form)
            _assert_parent(z, y, (form, "auto"))


# ---- the on-chip bound ----------------------------------------------------------------------------------------------------------------------------------
def test_the_on_chip_bound_is_served_refused_beyond_and_auto_falls_to_streamed(osg, gpu):
    L = osg._lib
    lib = L.vertical_diffusion_lib()
    bound = lib.tpg_vertical_diffusion_on_chip_levels(1, L.TPG_F64)
    assert bound >= 75                                             # the levels of the benchmark's grid
    at, beyond = ((2, 1, bound), (1, 1, 1), F64), ((2, 1, bound + 1), (1, 1, 1), F64)
    got = _run(osg, gpu, at, "profile", ON_CHIP, True)
    _assert_parent(got[0], _want(at, "profile", True)[0], "at the bound")
    h = _problem(beyond, "profile")
    args = ([_dev(h["fields"][0], gpu)], _dev(h["kappa"], gpu), R.PROFILE, _dev(h["dz_c"], gpu), _dev(h["dz_f"], gpu), None)
    for path in (ON_CHIP, AUTO):
        assert _solve(osg, gpu, *args, None, path, beyond[0], beyond[1]) == -5
        message = lib.tpg_vertical_diffusion_last_error().decode()
        assert f"Nz = {bound + 1} is beyond the on-chip path's {bound} levels" in message, message
    _assert_parent(args[0][0].cpu().numpy(), h["fields"][0], "a refused call writes nothing")
    for path in (AUTO, STREAMED):                                  # with scratch AUTO takes the streamed path
        got = _run(osg, gpu, beyond, "profile", path, True)
        _assert_parent(got[0], _want(beyond, "profile", True)[0], ("beyond the bound", path))


# ---- the elided division ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("path", PATHS)
def test_the_elided_division(osg, gpu, dtype, path):
    """kappa = -0.5, dz = 1, dt = 1, Nz = 2, f = (3, 7): beta is exactly 0 at level 2, the select takes f there, the result is (-1, 7)"""
    size, halo = (2, 1, 2), (1, 1, 1)
    f = np.full((4, 3, 4), np.nan, dtype)
    f[1, 1, 1:3], f[2, 1, 1:3] = 3, 7
    field, ones = _dev(f, gpu), _dev(np.ones(3, dtype), gpu)
    scratch = torch.empty_like(field)
    osg._lib.check_vertical_diffusion(_solve(osg, gpu, [field], None, R.CONSTANT, ones, ones, None, scratch, PATHS[path], size, halo, dt=1.0, kappa_value=-0.5))
    want = f.copy()
    want[1, 1, 1:3], want[2, 1, 1:3] = -1, 7
    _assert_parent(field.cpu().numpy(), want, "elided")
    assert np.array_equal(R.solve_column(np.array([3, 7], dtype), np.full(3, -0.5, dtype), np.ones(2, dtype), np.ones(3, dtype), 1.0), np.array([-1, 7], dtype))


# ---- special values -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("where", ["fields", "kappa", "both"])
def test_special_values(osg, gpu, dtype, where):
    """the pool of IEEE special values (signed zeros, subnormals, the extremes, infinities, NaN) in the fields, in kappa, and in both:
    the same bits as the reference, NaNs by NaN-ness, on both paths"""
    size, halo = (20, 10, 9), (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(7)
    shape = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    pool = sv.pool(dtype)
    f, kappa = np.full(shape, np.nan, dtype), np.full(shape, np.nan, dtype)
    f[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = sv.tiled(pool, (Nz, Ny, Nx)) if where != "kappa" else rng.uniform(-1, 1, (Nz, Ny, Nx))
    kappa[Hz + 1:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = (sv.tiled(np.roll(pool, 5), (Ny, Nz - 1, Nx)).transpose(1, 0, 2) if where != "fields"
                                                      else rng.uniform(0, 2, (Nz - 1, Ny, Nx)))
    dz_c, dz_f = rng.uniform(0.5, 2, Nz).astype(dtype), rng.uniform(0.5, 2, Nz + 1).astype(dtype)
    counts = _counts(size)
    want = R.reference([f], kappa, R.FIELD, dz_c, dz_f, DT, size, halo, counts, 0.0)[0]
    assert np.isnan(want[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]).any() and np.isfinite(want).any()
    for path in PATHS.values():
        field, scratch = _dev(f, gpu), _dev(np.full(shape, np.nan, dtype), gpu)
        osg._lib.check_vertical_diffusion(_solve(osg, gpu, [field], _dev(kappa, gpu), R.FIELD, _dev(dz_c, gpu), _dev(dz_f, gpu), _dev(counts, gpu),
                                                 scratch, path, size, halo))
        _assert_parent(field.cpu().numpy(), want, (where, path))


# ---- latitude bands -------------------------------------------------------------------------------------------------------------------------------------
def test_three_latitude_bands_give_the_rows_of_the_global_call(osg, gpu):
    case = ((20, 24, 5), (4, 4, 4), F64)
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h, counts = _problem(case, "field"), _counts(size)
    whole = _run(osg, gpu, case, "field", ON_CHIP, True)[0]
    _assert_parent(whole, _want(case, "field", True)[0], "global")
    for band in range(3):
        rows = slice(8 * band, 8 * band + 8 + 2 * Hy)              # the band's padded rows of the global parents
        field, kappa = (_dev(np.ascontiguousarray(a[:, rows]), gpu) for a in (h["fields"][0], h["kappa"]))
        osg._lib.check_vertical_diffusion(_solve(osg, gpu, [field], kappa, R.FIELD, _dev(h["dz_c"], gpu), _dev(h["dz_f"], gpu),
                                                 _dev(np.ascontiguousarray(counts[8 * band:8 * band + 8]), gpu), None, ON_CHIP, (Nx, 8, Nz), halo))
        _assert_parent(field.cpu().numpy()[:, Hy:Hy + 8], whole[:, Hy + 8 * band:Hy + 8 * band + 8], band)


# ---- the package ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,halo,tdt,path", [((48, 40, 6), (5, 5, 5), torch.float64, "auto"), ((50, 40, 3), (4, 4, 4), torch.float32, "streamed")],
                         ids=["48x40x6-h5-f64-auto", "50x40x3-h4-f32-streamed"])
def test_the_plan_equals_the_reference_and_replays_in_a_graph_with_dt(osg, gpu, size, halo, tdt, path):
    """on a built immersed grid with its own spacings and counts: the plan's fields are the reference's, it allocates nothing when called,
    with_dt gives the reference at the new step over the same tensors, and a captured graph replays the eager bits"""
    from gpu_harness import _grid
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = _grid(osg, size, halo, tdt, True)
    gen = torch.Generator(device=gpu).manual_seed(5)
    fields = [osg.CenterField(grid) for _ in range(2)]
    for f in fields:
        f.data.uniform_(-1, 1, generator=gen)
    start = [f.data.clone() for f in fields]
    kappa = torch.empty(Nz + 1, dtype=tdt, device=gpu).uniform_(0, 2, generator=gen)
    np_t = F64 if tdt == torch.float64 else F32
    dz_c = osg.z_center_spacings(grid, tdt).numpy().astype(np_t)
    dz_f = osg.z_all_face_spacings(grid, tdt).numpy().astype(np_t)
    counts = grid.column_counts["cc"].cpu().numpy()
    plan = osg.vertical_implicit_diffusion_plan(fields, kappa, DT, path=path)
    assert plan.scratch is not None and plan.scratch.shape == fields[0].data.shape       # "auto" and "streamed" hold a scratch parent
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    plan()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before              # the plan allocates nothing when called
    host = [t.cpu().numpy() for t in start]
    for f, w_ in zip(fields, R.reference(host, kappa.cpu().numpy(), R.PROFILE, dz_c, dz_f, DT, size, halo, counts, 0.0)):
        _assert_parent(f.data.cpu().numpy(), w_, "plan")
    half = plan.with_dt(DT / 2)
    assert half.dt == DT / 2 and plan.dt == DT and half.scratch is plan.scratch and half.fields is plan.fields
    for f, t in zip(fields, start):
        f.data.copy_(t)
    half()
    torch.cuda.synchronize()
    eager = [f.data.cpu().numpy() for f in fields]
    for g_, w_ in zip(eager, R.reference(host, kappa.cpu().numpy(), R.PROFILE, dz_c, dz_f, DT / 2, size, halo, counts, 0.0)):
        _assert_parent(g_, w_, "with_dt")
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            half()
    torch.cuda.current_stream().wait_stream(side)
    for f, t in zip(fields, start):
        f.data.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    for f, w_ in zip(fields, eager):
        _assert_parent(f.data.cpu().numpy(), w_, "replay")
    # the one-call form, a Field of kappa, and the model's three calls
    ku = osg.Field((osg.Face, osg.Center, osg.Face), grid)
    ku.data.uniform_(0, 2, generator=gen)
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (u, v, *fields):
        f.data.uniform_(-1, 1, generator=gen)
    hu, hv, hc = (f.data.cpu().numpy() for f in (u, v, fields[0]))
    osg.vertical_implicit_diffusion(u, ku, DT, path=path)
    kfaces = ku.data.cpu().numpy()[:Nz + 2 * Hz]
    _assert_parent(u.data.cpu().numpy(), R.reference([hu], kfaces, R.FIELD, dz_c, dz_f, DT, size, halo, grid.column_counts["fc"].cpu().numpy(), 0.0)[0], "u")
    u.data.copy_(torch.from_numpy(hu))
    closure = osg.VerticalScalarDiffusivity(osg.VerticallyImplicitTimeDiscretization(), nu=0.25, kappa={"T": 0.5, "S": 0.5})
    step = osg.implicit_step_plan(u, v, {"T": fields[0], "S": fields[1]}, closure, DT, path=path)
    assert len(step.plans) == 3                                    # u, v, and the two tracers of one kappa together
    assert all(p_.scratch is step.plans[0].scratch for p_ in step.plans)                  # one scratch parent for the step
    step()
    torch.cuda.synchronize()
    for f, h0, key, k in ((u, hu, "fc", 0.25), (v, hv, "cf", 0.25), (fields[0], hc, "cc", 0.5)):
        want = R.reference([h0], k, R.CONSTANT, dz_c, dz_f, DT, size, halo, grid.column_counts[key].cpu().numpy(), 0.0)[0]
        _assert_parent(f.data.cpu().numpy(), want, key)


# ---- past 2^31 elements -----------------------------------------------------------------------------------------------------------------------------------
def test_float32_constant_form_past_2g_elements(osg, gpu):
    """8640 x 4320 x 64, halo 4, Float32, CONSTANT form, masked: 2.69e9 elements in the parent.  Data drawn on the device.  The on-chip and the
    streamed call give the same bits (integer views, on the device); every halo cell keeps its value; and on windows of planes -- the four
    that hold the first cells at or past 2^31 and the top four -- strips of 16 rows equal the numpy reference of their columns (all 64
    levels of the strip go to the host: a column is solved whole).  Prints its wall time and peak device memory; the peak stays under half
    the card."""
    from gpu_harness import BIG, BIG_HALO, _big_counts, _cell_at, _random
    import tendency_windows as tw
    size, halo = BIG, BIG_HALO
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    shape = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    assert np.prod(shape, dtype=np.int64) == 2694855168
    k31, j31, _ = _cell_at(TWO31, size, halo)
    rng = np.random.default_rng(3)
    dz_c, dz_f = rng.uniform(0.5, 2, Nz).astype(F32), rng.uniform(0.5, 2, Nz + 1).astype(F32)
    with _budget(gpu, "vertical implicit diffusion"):
        start = _random(gpu, shape, 100, -1.0, 1.0)
        counts = _big_counts(gpu, size, 200)
        tables = _dev(dz_c, gpu), _dev(dz_f, gpu)
        a = start.clone()
        osg._lib.check_vertical_diffusion(_solve(osg, gpu, [a], None, R.CONSTANT, *tables, counts, None, ON_CHIP, size, halo, kappa_value=KAPPA))
        torch.cuda.synchronize()
        for dim, x in enumerate((Hz, Hy, Hx)):                     # the halos are as they were
            for lo in (0, shape[dim] - x):
                assert torch.equal(tw._ints(a.narrow(dim, lo, x)), tw._ints(start.narrow(dim, lo, x))), dim
        for which, lo in (("middle", min(max(j31 - 8, 0), Ny - 16)), ("top", Ny - 16)):
            strip = start[:, Hy + lo - Hy:Hy + lo + 16 + Hy].contiguous().cpu().numpy()
            want = R.reference([strip], KAPPA, R.CONSTANT, dz_c, dz_f, DT, (Nx, 16, Nz), halo, counts[lo:lo + 16].cpu().numpy(), 0.0)[0]
            got = a[:, lo:lo + 16 + 2 * Hy].contiguous().cpu().numpy()
            levels = range(k31 - 1, k31 + 3) if which == "middle" else range(Nz - 4, Nz)
            for k in levels:
                bad = same_bits(got[Hz + k, Hy:Hy + 16, Hx:Hx + Nx], want[Hz + k, Hy:Hy + 16, Hx:Hx + Nx])
                assert bad == 0, (which, k, bad)
            assert which != "middle" or (lo <= j31 < lo + 16 and (Hz + k31) * shape[1] * shape[2] <= TWO31)
            del strip, want, got
        scratch = torch.empty_like(start)
        osg._lib.check_vertical_diffusion(_solve(osg, gpu, [start], None, R.CONSTANT, *tables, counts, scratch, STREAMED, size, halo, kappa_value=KAPPA))
        torch.cuda.synchronize()
        for k0 in range(0, shape[0], 8):
            assert torch.equal(tw._ints(a[k0:k0 + 8]), tw._ints(start[k0:k0 + 8])), k0
        del a, start, scratch, counts


def test_the_example_steps_agree_eagerly_and_as_a_graph():
    """examples/vertical_diffusion_model_step.py asserts that its eager and replayed steps agree bit for bit"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "vertical_diffusion_model_step.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
