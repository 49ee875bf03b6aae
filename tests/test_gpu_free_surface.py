"""GPU tests of the split-explicit free-surface sub-step: tpg_free_surface_substep through the C ABI, and split_explicit_substep /
SplitExplicitFreeSurface / the sub-cycle plan through the package.  Compared BIT FOR BIT with tests/free_surface_ref.py (numpy in the
fields' type: every operation of the rule is one correctly rounded IEEE operation in one order, so the reference is exact and there is no
tolerance anywhere in this file); NaNs compare by NaN-ness; no case and no cell is left out of a comparison.

Shapes (size, Hx, Hy2, type): the smallest at which each path can go wrong.  A work item is one chunk (2 doubles, 4 floats, 2 floats where
Nx = 2 mod 4) x 2 rows (4 and 8 in the recorded variants): rows of one, two and three chunks; Ny = 2, 3, 4, 5, 9 (at and one past the rows of
an item for 2, 4 and 8 rows; below them is Ny = 1, which the call refuses); halo 4 (16-B
chunks) and halo 5 or 1 (element-aligned chunks); Hy2 from 1 to config 5's 31; one shape with more work items than are resident.  Every
case runs with every pointer on the 16-B grid and one element past an allocation, with and without count planes (land columns among them),
with and without averaging.  The metrics are random in [0.5, 2] and depth_of_count random positive, so a wrong index cannot hide."""

import numpy as np
import pytest
import torch

import barotropic_ref
import free_surface_ref as ref
from free_surface_ref import METRICS, same_bits
from gpu_harness import _dev, _free_hbm  # noqa: F401
from immersed_ref import draw_columns, heights_of
from special_values import pool

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
#         size          Hx Hy2  element type
TABLE = [((2, 2, 1), 1, 1, F64),                   # one chunk, two rows, the thinnest halos
         ((4, 3, 2), 4, 2, F64),                   # two chunks; Ny one past the rows of an item
         ((6, 4, 3), 5, 3, F64),                   # three chunks; two whole items of rows; odd Hx: element-aligned chunks
         ((4, 5, 3), 4, 6, F32),                   # one 16-B chunk; two items of rows and one row
         ((8, 4, 3), 5, 2, F32),                   # two chunks, odd Hx
         ((12, 9, 3), 4, 13, F32),                 # three chunks; the reference's 12-substep extended halo
         ((6, 5, 3), 4, 4, F32),                   # Nx = 2 mod 4: three 8-B chunks
         ((48, 40, 6), 5, 31, F64),                # the model halo with config 5's Hy2
         ((50, 40, 3), 4, 13, F32),
         ((1536, 1283, 2), 4, 4, F64)]             # 321 x 768 items, 963 blocks: more than are resident
SENTINEL = 12345.0
DTAU, G, WEIGHT = 0.3, 9.80665, 0.1                # none representable: each is converted once to the field type
STATE, FORCING, BARS = ("eta", "U", "V"), ("GU", "GV"), ("eta_bar", "U_bar", "V_bar")
PLANES = STATE + FORCING + BARS + METRICS


def _id(case):
    size, Hx, Hy2, dtype = case
    return "x".join(map(str, size)) + f"-h{Hx}-{Hy2}" + ("-f64" if dtype == F64 else "-f32")


_CASES = {}


def _case(case):
    """host arrays of a case, random in EVERY cell (halos included): the state, the forcing, the averages, the five metrics, depth_of_count,
    two count planes (land columns, open columns, everything between, one count above Nz and one below 0); and the reference interiors with
    and without the planes.  Computed once per case, shared by the tests, never modified (tests copy what they change)"""
    if case not in _CASES:
        size, Hx, Hy2, dtype = case
        Nx, Ny, Nz = size
        shape = (Ny + 2 * Hy2, Nx + 2 * Hx)
        rng = np.random.default_rng([*size, Hx, Hy2, np.dtype(dtype).itemsize])
        h = {k: rng.uniform(-1, 1, shape).astype(dtype) for k in STATE + FORCING + BARS}
        h.update({k: rng.uniform(0.5, 2, shape).astype(dtype) for k in METRICS})
        h["depth"] = rng.uniform(0.5, 2, Nz + 1).astype(dtype)
        for k in ("n_fc", "n_cf"):
            n = (draw_columns(rng, Nx, Ny, Nz) if Nx >= 24 else rng.integers(0, Nz + 1, (Ny, Nx))).astype(np.int32)
            n[0, 0], n[Ny - 1, Nx - 1], n[Ny - 1, 0] = Nz, Nz + 3, -2
            h[k] = n
        h["want"] = {c: _interiors(h, size, Hx, Hy2, c) for c in (False, True)}
        for a in h.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[case] = h
    return _CASES[case]


def _interiors(h, size, Hx, Hy2, counts):
    n = (h["n_fc"], h["n_cf"]) if counts else (None, None)
    return ref.interior_substep(*(h[k] for k in STATE + FORCING), {k: h[k] for k in METRICS}, h["depth"], size, Hx, Hy2, DTAU, G, *n)


def _want(h, new, size, Hx, Hy2, avg):
    """whole planes: the outputs from sentinel-filled ones, the averages from h's (None without averaging)"""
    Nx, Ny, _ = size
    T = h["depth"].dtype
    inner = (slice(Hy2, Hy2 + Ny), slice(Hx, Hx + Nx))
    outs = []
    for x in new:
        p = np.full(h["eta"].shape, SENTINEL, T)
        p[inner] = x
        outs.append(p)
    if not avg:
        return outs, None
    bars = []
    for k, x in zip(BARS, new):
        b = h[k].copy()
        with np.errstate(all="ignore"):
            b[inner] = h[k][inner] + T.type(WEIGHT) * x
        bars.append(b)
    return outs, bars


def _ptr(t):
    return None if t is None else t.data_ptr()


def _substep(osg, gpu, h, size, Hx, Hy2, counts=False, avg=False, offset=0, n=None):
    """tpg_free_surface_substep on device copies of h into fresh sentinel-filled outputs -> (the whole output planes, the whole averages
    or None) on the host"""
    T = h["depth"].dtype
    d = {k: _dev(h[k], gpu, offset) for k in PLANES if avg or k not in BARS}
    outs = [_dev(np.full(h["eta"].shape, SENTINEL, T), gpu, offset) for _ in range(3)]
    depth = _dev(h["depth"], gpu, offset)
    n = n if n is not None else ((h["n_fc"], h["n_cf"]) if counts else (None, None))
    nd = [None if p is None else _dev(p, gpu, offset) for p in n]
    osg._lib.check_free_surface(osg._lib.free_surface_lib().tpg_free_surface_substep(
        *(t.data_ptr() for t in outs), *(d[k].data_ptr() for k in STATE + FORCING), *(_ptr(d.get(k)) for k in BARS),
        *(d[k].data_ptr() for k in METRICS), depth.data_ptr(), _ptr(nd[0]), _ptr(nd[1]), DTAU, G, WEIGHT, *size, Hx, Hy2,
        osg._lib.ft_of(depth.dtype), osg._lib.current_stream_ptr(gpu)))
    return [t.cpu().numpy() for t in outs], ([d[k].cpu().numpy() for k in BARS] if avg else None)


def _assert_same(got, want, what):
    bad = same_bits(got, want)
    assert bad == 0, (what, bad, "cells differ of", got.size)


def _assert_call(osg, gpu, h, new, size, Hx, Hy2, counts, avg, offset, what, n=None):
    outs, bars = _substep(osg, gpu, h, size, Hx, Hy2, counts, avg, offset, n)
    want_outs, want_bars = _want(h, new, size, Hx, Hy2, avg)
    for k, g, w in zip(STATE, outs, want_outs):
        _assert_same(g, w, (what, k, counts, avg))
    if avg:
        for k, g, w in zip(BARS, bars, want_bars):
            _assert_same(g, w, (what, k, counts, avg))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_whole_planes_are_bit_exact_and_only_interiors_are_written(osg, gpu, case, offset):
    """random data in every cell.  The outputs pre-filled with a sentinel equal the reference's -- the interior the rule, every halo cell
    still the sentinel; the averages equal the reference's -- the interior with weight x the new state added, every halo cell its random
    value.  With and without count planes, with and without averaging, and with one count plane only"""
    size, Hx, Hy2, dtype = case
    Nx, Ny, Nz = size
    h = _case(case)
    for c in (False, True):                                        # the references themselves: row 1 of V carried, everything else moved
        eta, U, V = h["want"][c]
        inner = (slice(Hy2, Hy2 + Ny), slice(Hx, Hx + Nx))
        assert same_bits(V[0], h["V"][inner][0]) == 0 and (V[1:] != h["V"][inner][1:]).mean() > 0.9
        assert (eta != h["eta"][inner]).mean() > 0.9 and (U != h["U"][inner]).mean() > 0.9
    assert same_bits(h["want"][False][1], h["want"][True][1]) > 0 and (h["n_fc"] >= Nz).any() and (h["n_cf"] >= Nz).any()
    for counts in (False, True):
        for avg in (False, True):
            _assert_call(osg, gpu, h, h["want"][counts], size, Hx, Hy2, counts, avg, offset, "substep")
    one = ref.interior_substep(*(h[k] for k in STATE + FORCING), {k: h[k] for k in METRICS}, h["depth"], size, Hx, Hy2, DTAU, G, None, h["n_cf"])
    _assert_call(osg, gpu, h, one, size, Hx, Hy2, True, True, offset, "n_cf only", n=(None, h["n_cf"]))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_no_cell_outside_the_rule_is_read(osg, gpu, case, offset):
    """every cell the rule does not read is NaN -- every halo cell but U's and dy_fc's east column and V's and dx_cf's north row, row 1 of
    GV and dy_cf, the halos of the averages, the entries of depth_of_count no count selects: the results have no NaN and equal the clean
    ones"""
    size, Hx, Hy2, dtype = case
    h = _case(case)
    read = ref.cells_read(size, Hx, Hy2, h["n_fc"], h["n_cf"])
    nan = dtype(np.nan)
    poisoned = {k: np.where(read["average" if k in BARS else k], h[k], nan) for k in PLANES}
    poisoned["depth"] = np.where(read["depth_of_count"], h["depth"], nan)
    poisoned["n_fc"], poisoned["n_cf"] = h["n_fc"], h["n_cf"]
    assert all(np.isnan(poisoned[k]).sum() == (~read["average" if k in BARS else k]).sum() > 0 for k in PLANES)
    outs, bars = _substep(osg, gpu, poisoned, size, Hx, Hy2, True, True, offset)
    want_outs, want_bars = _want(h, h["want"][True], size, Hx, Hy2, True)
    inner = read["eta"]
    for k, g, w in zip(STATE, outs, want_outs):
        assert not np.isnan(g).any()
        _assert_same(g, w, ("poisoned", k))
    for k, g, w in zip(BARS, bars, want_bars):
        assert not np.isnan(g[inner]).any() and np.isnan(g[~inner]).all()
        _assert_same(g[inner], w[inner], ("poisoned", k))
    # without planes: entry 0 of depth_of_count alone
    poisoned["depth"] = np.where(np.arange(size[2] + 1) == 0, h["depth"], nan)
    outs, _ = _substep(osg, gpu, poisoned, size, Hx, Hy2, False, False, offset)
    for k, g, w in zip(STATE, outs, _want(h, h["want"][False], size, Hx, Hy2, False)[0]):
        _assert_same(g, w, ("poisoned, no planes", k))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", TABLE, ids=_id)
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max planted in 2 % of the cells of the state, the forcing and the averages (at least one each), one NaN
    and one +Inf explicitly in the interior, a zero and a negative-zero metric, depth_of_count = +-0 for one count each: bit for bit numpy's,
    which computes the same IEEE operations -- NaN / Inf patterns and the sign of zero included"""
    size, Hx, Hy2, dtype = case
    Nx, Ny, Nz = size
    h = dict(_case(case))
    rng = np.random.default_rng([7, *size, Hx, Hy2])
    p = pool(dtype)
    for name in STATE + FORCING + BARS:
        a = h[name].copy()
        where = rng.random(a.shape) < 0.02
        where[Hy2 + rng.integers(0, Ny), Hx + rng.integers(0, Nx)] = True
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
        h[name] = a
    h["eta"][Hy2, Hx], h["U"][Hy2 + 1, Hx + 1] = np.nan, np.inf
    for k, (j, i) in (("az_cc", (1, 0)), ("dx_fc", (0, 0)), ("dy_cf", (1, 1))):
        h[k] = h[k].copy()
        h[k][Hy2 + j, Hx + i] = 0.0
        h[k][Hy2, Hx + Nx - 1] = -0.0
    depth = h["depth"].copy()
    depth[Nz] = 0.0                                                # a land column's depth: H = 0 only drops the pressure term
    if Nz > 1:
        depth[1] = -0.0
    h["depth"] = depth
    for counts in (False, True):
        new = _interiors(h, size, Hx, Hy2, counts)
        assert any(np.isnan(x).any() for x in new)
        _assert_call(osg, gpu, h, new, size, Hx, Hy2, counts, True, offset, "special values")
    # the zeros alone, on clean data: Inf and NaN from the divisions, the sign of zero from the land columns
    clean = dict(_case(case))
    clean.update({k: h[k] for k in ("az_cc", "dx_fc", "dy_cf", "depth")})
    new = _interiors(clean, size, Hx, Hy2, True)
    assert not np.isfinite(new[0]).all()
    _assert_call(osg, gpu, clean, new, size, Hx, Hy2, True, False, offset, "zero metrics")


def test_lake_at_rest_and_the_sign_of_zero(osg, gpu):
    """eta constant, U = V = G = 0 through the C ABI: eta stays the constant, U and V stay +0 -- and with U = V = -0 the rule's own zeros"""
    size, Hx, Hy2, dtype = (12, 9, 3), 4, 13, F32
    h = dict(_case((size, Hx, Hy2, dtype)))
    shape = h["eta"].shape
    for zero in (0.0, -0.0):
        h.update(eta=np.full(shape, 0.37, dtype), U=np.full(shape, zero, dtype), V=np.full(shape, zero, dtype), GU=np.zeros(shape, dtype),
                 GV=np.zeros(shape, dtype))
        new = _interiors(h, size, Hx, Hy2, True)
        assert (new[0] == dtype(0.37)).all() and (new[1] == 0).all() and (new[2] == 0).all()
        _assert_call(osg, gpu, h, new, size, Hx, Hy2, True, True, 0, "lake at rest")


def test_every_error_return_leaves_the_outputs_untouched(osg, gpu):
    """real device arrays, one argument wrong at a time: the status is negative and eta_out, U_out, V_out and the averages hold what they held"""
    size, Hx, Hy2, dtype = (12, 9, 3), 4, 13, F32
    h = _case((size, Hx, Hy2, dtype))
    lib = osg._lib.free_surface_lib()
    outs = [_dev(np.full(h["eta"].shape, SENTINEL, dtype), gpu) for _ in range(3)]
    d = {k: _dev(h[k], gpu) for k in PLANES}
    depth, nfc, ncf = _dev(h["depth"], gpu), _dev(h["n_fc"], gpu), _dev(h["n_cf"], gpu)
    names = ("eta_out", "U_out", "V_out") + STATE + FORCING + BARS + METRICS + ("depth", "n_fc", "n_cf")
    good = dict(zip(names, [t.data_ptr() for t in outs] + [d[k].data_ptr() for k in PLANES] + [depth.data_ptr(), nfc.data_ptr(), ncf.data_ptr()]))
    geom = dict(Nx=size[0], Ny=size[1], Nz=size[2], Hx=Hx, Hy2=Hy2, ft=osg._lib.TPG_F32)

    def call(ptrs=None, **kw):
        p, g = {**good, **(ptrs or {})}, {**geom, **kw}
        return lib.tpg_free_surface_substep(*(p[k] for k in names), DTAU, G, WEIGHT, g["Nx"], g["Ny"], g["Nz"], g["Hx"], g["Hy2"], g["ft"],
                                            osg._lib.current_stream_ptr(gpu))
    wrong = [call(ft=7), call(Nx=11), call(Hx=0), call(Hy2=0), call(Ny=1)]
    wrong += [call({k: None}) for k in names[:8] + names[11:17]]                       # a NULL required pointer
    wrong += [call({k: None}) for k in BARS] + [call({BARS[0]: None, BARS[2]: None})]  # a half-given averaging triple
    wrong += [call({k: good[k] + 2}) for k in names]                                    # off the element / int32 alignment
    wrong += [call({"eta_out": good["eta"]}), call({"U_out": good["U"]}), call({"V_out": good["V"]}), call({"eta_out": good["U_out"]}),
              call({"eta_bar": good["eta_out"]}), call({"U_bar": good["dx_fc"] + 4}), call({"V_out": good["depth"]}), call({"V_bar": good["n_cf"]})]
    assert all(rc in (-1, -2, -5) for rc in wrong), wrong
    assert wrong[:5] == [-1, -2, -1, -1, -5]
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all())
    for k in BARS:
        _assert_same(d[k].cpu().numpy(), h[k], ("untouched", k))
    osg._lib.check_free_surface(call())                            # and the same arrays, all arguments right: the rule
    _, want_bars = _want(h, h["want"][True], size, Hx, Hy2, True)
    for k, w in zip(BARS, want_bars):
        _assert_same(d[k].cpu().numpy(), w, ("then the call", k))


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
def _np_type(tdt):
    return F64 if tdt == torch.float64 else F32


def _host_metrics(ext):
    return {k: ext.arrays[k].cpu().numpy() for k in METRICS}


def _filled(osg, like, interior, base):
    """the parent fill_halo_regions gives a field at `like`'s location and grid that held `base` (a (1, sy, sx) array) and got that interior"""
    f = osg.Field(like.loc, like.grid)
    f.data.copy_(torch.from_numpy(np.ascontiguousarray(base)).reshape(f.data.shape))
    f.interior().copy_(torch.from_numpy(np.ascontiguousarray(interior)).reshape(f.interior().shape))
    osg.fill_halo_regions([f])
    return f.data.cpu().numpy()


def _randomize(osg, gpu, fs, seed, scale=1.0):
    """random state and forcing in every cell, then the halos of the state filled (the first sub-step reads them); the twins and the
    averages random too: the plan owes nothing to what they held"""
    gen = torch.Generator(device=gpu).manual_seed(seed)
    for f in (*fs.state, fs.GU, fs.GV, *fs.twins, *fs.averages):
        f.data.uniform_(-scale, scale, generator=gen)
    osg.fill_halo_regions(list(fs.state))


def _reference_subcycle(osg, fs, dtau, n_fc=None, n_cf=None, average=True):
    """the sub-cycle on the host from the free surface's device state: the reference sub-step alternated with the project's own fill, on the
    two sets of whole parents as the plan uses them -> (state parents, twin parents, average parents or None)"""
    ext = fs.extended_grid
    T = _np_type(ext.dtype)
    size, Hx, Hy2 = (ext.Nx, ext.Ny, ext.Nz), ext.Hx, ext.Hy
    sets = [[f.data.cpu().numpy() for f in fs.state], [f.data.cpu().numpy() for f in fs.twins]]
    Gs = [f.data[0].cpu().numpy() for f in (fs.GU, fs.GV)]
    metrics = _host_metrics(ext)
    depth = osg.column_depth_table(ext, ext.dtype).numpy().astype(T)
    inner = (0, slice(Hy2, Hy2 + ext.Ny), slice(Hx, Hx + ext.Nx))
    bars = [np.zeros_like(a) for a in sets[0]] if average else None
    copy_first, steps = (fs.substeps % 2 == 1), []
    if copy_first:
        sets[1] = [a.copy() for a in sets[0]]
    src = 1 if copy_first else 0
    for s in range(fs.substeps):
        new = ref.interior_substep(*(a[0] for a in sets[src]), *Gs, metrics, depth, size, Hx, Hy2, dtau, fs.gravitational_acceleration, n_fc, n_cf)
        dst = 1 - src
        sets[dst] = [_filled(osg, f, x, base) for f, x, base in zip(fs.state, new, sets[dst])]
        if average:
            for b, x in zip(bars, new):
                b[inner] = b[inner] + T(fs.weights[s]) * x
        src = dst
    assert src == 0                                                # the final state is in the caller's fields
    if average:
        bars = [_filled(osg, f, b[inner], b) for f, b in zip(fs.state, bars)]
    return sets[0], sets[1], bars


def _assert_free_surface(fs, want, what):
    state, twins, bars = want
    for f, w in zip(fs.state, state):
        _assert_same(f.data.cpu().numpy(), w, (what, "state", f.name))
    for f, w in zip(fs.twins, twins):
        _assert_same(f.data.cpu().numpy(), w, (what, "twin", f.name))
    if bars is not None:
        for f, w in zip(fs.averages, bars):
            _assert_same(f.data.cpu().numpy(), w, (what, "average", f.name))


@pytest.mark.parametrize("substeps", [1, 2, 3])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 3), (4, 4, 4), torch.float64), ((50, 40, 3), (5, 5, 5), torch.float32)], ids=["48x40-h4-f64", "50x40-h5-f32"])
def test_subcycle_plan_equals_the_reference_alternated_with_the_fill(osg, gpu, size, halo, tdt, substeps):
    """1, 2 and 3 sub-steps (odd: the twins take a copy of the state first) with non-uniform weights: whole filled parents of the state, the
    twins and the averages; the plan allocates nothing when called; then the same plan replayed from a graph on a new state"""
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
    weights = [0.5, 0.3, 0.2][:substeps]
    fs = osg.SplitExplicitFreeSurface(grid, substeps=substeps, weights=weights)
    assert fs.extended_grid is grid and fs.eta.Hy == halo[1]       # substeps + 1 <= Hy: the grid's own halo is wide enough
    _randomize(osg, gpu, fs, 3)
    want = _reference_subcycle(osg, fs, DTAU)
    plan = osg.split_explicit_subcycle_plan(fs, DTAU)
    assert plan.schedule[-1][1] == 0 and len(plan.schedule) == substeps
    assert plan() is plan
    _assert_free_surface(fs, want, "eager")
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
    _randomize(osg, gpu, fs, 17)
    want = _reference_subcycle(osg, fs, DTAU)
    graph.replay()
    torch.cuda.synchronize()
    _assert_free_surface(fs, want, "replay")
    # without averaging the averages stay as they were
    held = [f.data.clone() for f in fs.averages]
    _randomize(osg, gpu, fs, 19)
    for f, t in zip(fs.averages, held):
        f.data.copy_(t)
    want = _reference_subcycle(osg, fs, DTAU, average=False)
    osg.split_explicit_subcycle_plan(fs, DTAU, average=False)()
    _assert_free_surface(fs, (want[0], want[1], [t.cpu().numpy() for t in held]), "no averaging")


def test_extended_halo_and_one_substep_through_the_package(osg, gpu):
    """12 sub-steps on a halo-4 grid: the fields live on with_halo((4, 13, 4), grid); split_explicit_substep is one call of the rule with
    that grid's metrics and writes no halo cell"""
    size, halo = (48, 40, 3), (4, 4, 4)
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo, z=(-1, 0))
    fs = osg.SplitExplicitFreeSurface(grid, substeps=12)
    ext = fs.extended_grid
    assert ext is not grid and (ext.Hx, ext.Hy, ext.Hz) == (4, 13, 4) and fs.eta.Hy == 13 and tuple(fs.V.data.shape) == (1, 40 + 26, 48 + 8)
    assert fs.weights == [1 / 12] * 12
    _randomize(osg, gpu, fs, 5)
    for f in fs.twins:
        f.data.fill_(SENTINEL)
    host = [f.data[0].cpu().numpy() for f in (*fs.state, fs.GU, fs.GV)]
    bars0 = [f.data[0].cpu().numpy() for f in fs.averages]
    depth = osg.column_depth_table(ext, torch.float64).numpy()
    out0 = [np.full(host[0].shape, SENTINEL, F64) for _ in range(3)]
    outs, bars = ref.substep(out0, host[:3], host[3:], _host_metrics(ext), depth, size, 4, 13, DTAU, 9.81, averages=bars0, weight=WEIGHT)
    got = osg.split_explicit_substep(*fs.twins, *fs.state, fs.GU, fs.GV, DTAU, gravitational_acceleration=9.81, averages=fs.averages, weight=WEIGHT)
    assert got[0] is fs.twins[0] and got[2] is fs.twins[2]
    for f, w in zip(fs.twins, outs):
        _assert_same(f.data[0].cpu().numpy(), w, ("substep", f.name))
    for f, w in zip(fs.averages, bars):
        _assert_same(f.data[0].cpu().numpy(), w, ("substep average", f.name))
    # lake at rest through the plan: eta constant, U = V = G = 0 stays exactly so after 12 sub-steps and their fills.  The tripolar grid
    # has two (Face, Center) nodes with a zero metric beside the poles, where the rule divides 0 by 0 (a model has land there; the free
    # surface's mask is out of scope): this free surface's own grid gets a non-zero metric in those cells first
    zeros = 0
    for k in METRICS:
        a = ext.arrays[k]
        zeros += int((a[ext.Hy:ext.Hy + ext.Ny, ext.Hx:ext.Hx + ext.Nx] == 0).sum())
        a[a == 0] = 1.0
    assert zeros > 0
    for f in (*fs.state, fs.GU, fs.GV, *fs.twins):
        f.data.zero_()
    fs.eta.data.fill_(0.37)
    osg.split_explicit_subcycle_plan(fs, 40.0)()
    assert bool((fs.eta.data == 0.37).all()) and bool((fs.twins[0].data[0, ext.Hy:] == 0.37).all())      # the twin's south halo: its fill's
    for f in (fs.U, fs.V, *fs.twins[1:], fs.U_bar, fs.V_bar):
        assert bool((f.data == 0).all()), f.name                   # the fold writes -0 into the halos and the east half of row Ny: zero all the same
    acc = F64(0)
    for w in fs.weights:                                           # 12 additions of (1 / 12) * 0.37, in the rule's order
        acc = acc + F64(w) * F64(0.37)
    assert bool((fs.eta_bar.data[0, ext.Hy:] == float(acc)).all()) and bool((fs.eta_bar.data[0, :ext.Hy] == 0).all())    # the south halo has no condition: the zeros


def test_mode_subcycle_correction_chain_on_an_immersed_grid(osg, gpu):
    """compute_barotropic_mode -> the 5-sub-step plan -> barotropic_correction on an ImmersedBoundaryGrid, against the references chained:
    the count planes select the column depths in every sub-step (land columns keep their transport but for the forcing) and mask the
    corrected velocities"""
    size, halo = (48, 40, 6), (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    base = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo, z=(-1, 0))
    zc = base.z_centers[Hz:Hz + Nz].cpu().numpy()
    rng = np.random.default_rng(19)
    ibg = osg.ImmersedBoundaryGrid(base, osg.GridFittedBottom(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)))
    nfc, ncf = (ibg.column_counts[k].cpu().numpy() for k in ("fc", "cf"))
    assert (nfc >= Nz).any() and (nfc == 0).any() and ((nfc > 0) & (nfc < Nz)).any()
    gen = torch.Generator(device=gpu).manual_seed(3)
    u, v = osg.XFaceField(ibg), osg.YFaceField(ibg)
    for f in (u, v):
        f.data.uniform_(-1, 1, generator=gen)
    fs = osg.SplitExplicitFreeSurface(ibg, substeps=5)
    ext = fs.extended_grid
    assert ext.Hy == 6 and fs.grid is ibg
    _randomize(osg, gpu, fs, 4, scale=0.01)
    Ub, Vb = osg.Field(fs.U.loc, ext, name="Ubar"), osg.Field(fs.V.loc, ext, name="Vbar")
    osg.compute_barotropic_mode(u, v, Ub, Vb)
    fs.U.data.copy_(Ub.data)
    fs.V.data.copy_(Vb.data)
    host_u, host_v = u.data.cpu().numpy(), v.data.cpu().numpy()
    dz = osg.z_center_spacings(base, torch.float64).numpy()
    for f, hf in ((Ub, host_u), (Vb, host_v)):                     # the mode, as tests/barotropic_ref.py states it, and its fill
        _assert_same(f.data.cpu().numpy(), _filled(osg, f, barotropic_ref.interior_mode(hf, dz, size, halo), np.zeros(tuple(f.data.shape))), ("mode", f.name))
    want = _reference_subcycle(osg, fs, 0.05, nfc, ncf)
    plain = _reference_subcycle(osg, fs, 0.05)
    assert same_bits(want[0][1], plain[0][1]) > 0                   # the count planes matter
    osg.split_explicit_subcycle_plan(fs, 0.05)()
    _assert_free_surface(fs, want, "immersed sub-cycle")
    osg.barotropic_correction(u, v, fs.U, fs.V, Ub, Vb)
    depth = osg.column_depth_table(base, torch.float64).numpy()
    for f, hf, t, tb, n in ((u, host_u, want[0][1], Ub, nfc), (v, host_v, want[0][2], Vb, ncf)):
        c = barotropic_ref.interior_correction(hf, t[0], tb.data[0].cpu().numpy(), depth, size, halo, ext.Hy, n, 0.0)
        w = osg.Field(f.loc, ibg, data=torch.from_numpy(hf).to(gpu))
        w.interior().copy_(torch.from_numpy(c))
        osg.fill_halo_regions([w])
        _assert_same(f.data.cpu().numpy(), w.data.cpu().numpy(), ("corrected", f.name))
