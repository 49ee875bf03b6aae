"""GPU tests of the tracer tendency of `WENO()` -- WENO5 in x, y and z, walls in z: tpg_weno_xyz_tracer_advection_tendency through the C
ABI, and weno_xyz_tracer_advection_tendency / weno_xyz_tracer_advection_plan through the package.  Compared BIT FOR BIT with
tests/weno_xyz_ref.py (numpy in the fields' type: every operation of the rule is one correctly rounded IEEE operation, so the reference is
exact and there is no tolerance anywhere in this file); NaNs compare by NaN-ness; whole parents are compared: the halo cells of G against a
sentinel.

Shapes: the horizontal sizes, halos and types of tests/test_gpu_weno.py's SMALL list (the chunk forms: the minimum halo, Float32 chunks wider
than Hx, 8-B chunks, Ny odd, the model halo, 63 and 64 chunks a row) crossed with Nz in {1, 2, 3, 4, 5, 6, 7, 9}: one level (two centred
faces), the levels at which the orders 1, 3 and 5 first appear, one more of each, and nine (three faces of order 5 in a row: the window has
moved through all its slots).  dz_c and the metrics are random in [0.5, 2], u, v, w of both signs -- w in every column and chunk."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import gpu_harness as H
import tendency_windows as tw
from gpu_harness import (F32, F64, MASK_VALUE, SENTINEL, _assert_parent, _count_plane, _dev, _free_hbm, _host_model, _id,  # noqa: F401
                         _tracer_model as _model)
from special_values import pool
from weno_xyz_ref import cells_read, dependence_window, face_order, same_bits, tendency

pytestmark = pytest.mark.gpu

KERNEL = tw.KERNELS["weno_xyz"]
LEVELS = (1, 2, 3, 4, 5, 6, 7, 9)
#          (Nx, Ny)   halo       element type
FORMS = [((10, 10), (4, 4, 4), F64),               # two chunk rows of five
         ((20, 12), (3, 3, 1), F64),               # the minimum halo: every stencil arm ends on the last halo cell
         ((20, 12), (3, 3, 1), F32),               # 16-B chunks wider than Hx: the plain form
         ((22, 6), (3, 3, 1), F32),                # 8-B chunks, Hx = 3: the chunk past the row's end fills the halo, its east reads are clamped
         ((20, 11), (4, 4, 4), F64),               # Ny odd: the last row tile is a partial one
         ((24, 11), (4, 4, 4), F32),               # the same on Float32 rows that sit on the 16-B grid
         ((48, 40), (5, 5, 5), F64),               # the model halo: the element-aligned chunks
         ((48, 40), (5, 5, 5), F32),
         ((50, 40), (4, 4, 4), F32),               # Nx = 2 mod 4: 8-B chunks
         ((126, 5), (4, 4, 4), F64),               # 63 chunks a row: one full wave, its last lane the chunk past the end
         ((128, 5), (3, 3, 1), F64),               # 64 chunks a row: the last chunk and the one past the end in a wave of their own
         ((252, 5), (4, 4, 4), F32)]               # 63 chunks of 16 B
CASES = [((nx, ny, nz), halo, dtype) for (nx, ny), halo, dtype in FORMS for nz in LEVELS]
OFFSET = [((20, 11, 9), (4, 4, 4), F64), ((48, 40, 6), (5, 5, 5), F64), ((50, 40, 7), (4, 4, 4), F32)]   # every pointer one element off the 16-B grid
NTRACERS = 3
SHARED = ("u", "v", "w", "dy_fc", "dx_cf", "az_cc", "dz_c")


def _ref(h, c, size, halo, n_cc=None):
    """the reference parent of G of the tracer `c` from a sentinel-filled one; with a count plane: masked to MASK_VALUE"""
    return H._ref(KERNEL, h, size, halo, () if n_cc is None else (n_cc,), c)


def _case(case, ntracers=NTRACERS):
    return H._case(KERNEL, case, ntracers)


def _device(h, gpu, offset=0):
    return H._device(KERNEL, h, gpu, offset)


def _raw_call(osg, gpu, d, tracers, outs, size, halo, n_cc=None, value=0.0):
    return H._launch(osg, gpu, KERNEL, dict(d, c=tracers), {"G": outs}, size, halo, counts=(n_cc,), value=value)


def _call(osg, gpu, d, size, halo, which=None, n_cc=None, value=0.0, offset=0, library="weno_xyz"):
    """the call (of `library`: this tendency's, or the x-y one's) on the tracers `which` (indices; None: all) of the device arrays d into
    fresh sentinel-filled outputs -> the whole parents of G on the host"""
    return H._call(osg, gpu, tw.KERNELS[library], d, size, halo, which, (n_cc,), value, offset)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,offset", [(c, 0) for c in CASES] + [(c, 1) for c in OFFSET],
                         ids=[_id(c) for c in CASES] + [_id(c) + "-offset" for c in OFFSET])
def test_interior_is_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, offset):
    """random data in every cell -- w of both signs inside every chunk and every column --, the parents of G pre-filled with a sentinel:
    with 1, 2 and 3 tracers in a call the whole parents equal the reference's -- the interior the rule, every halo cell still the sentinel"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    wi = h["w"][Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx]
    assert ((wi[:, :, 0::2] > 0) != (wi[:, :, 1::2] > 0)).any()   # both signs inside one chunk
    assert Nz < 4 or ((wi > 0).any(axis=0) & (wi < 0).any(axis=0)).mean() > 0.5      # and inside one column
    for want in h["want"]:                                         # the reference parents themselves: sentinel exactly on the halo cells
        edge = np.ones(want.shape, bool)
        edge[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
        assert (want[edge] == SENTINEL).all() and not (want[~edge] == SENTINEL).any() and np.isfinite(want).all()
    d = _device(h, gpu, offset)
    for n in (1, 2, 3):
        got = _call(osg, gpu, d, size, halo, which=range(n), offset=offset)
        for q in range(n):
            _assert_parent(got[q], h["want"][q], ("parent", n, q))
    for k in SHARED:                                               # the inputs come back as they were
        _assert_parent(d[k].cpu().numpy(), h[k], ("input", k))
    _assert_parent(d["c"][0].cpu().numpy(), h["c"][0], "input tracer 0")


@pytest.mark.parametrize("case", [((20, 11, 9), (4, 4, 4), F64), ((24, 11, 5), (4, 4, 4), F32)], ids=_id)
def test_seventeen_tracers_in_calls_of_sixteen_and_one(osg, gpu, case):
    """16 tracers in one call and the 17th in a call of its own, against the reference and against calls of one tracer"""
    size, halo, dtype = case
    h = _case(case, 17)
    d = _device(h, gpu)
    together = _call(osg, gpu, d, size, halo, which=range(16)) + _call(osg, gpu, d, size, halo, which=(16,))
    for q in range(17):
        _assert_parent(together[q], h["want"][q], ("17 tracers", q))
    for q in (0, 7, 15):
        _assert_parent(_call(osg, gpu, d, size, halo, which=(q,))[0], together[q], ("one by one", q))


@pytest.mark.parametrize("form", FORMS, ids=lambda f: _id(((*f[0], 1), f[1], f[2])))
def test_one_level_equals_the_existing_call(osg, gpu, form):
    """Nz = 1, two centred faces: bit for bit tpg_weno_tracer_advection_tendency on the same arrays -- no oracle"""
    (nx, ny), halo, dtype = form
    size = (nx, ny, 1)
    h = _case((size, halo, dtype))
    d = _device(h, gpu)
    new, old = _call(osg, gpu, d, size, halo), _call(osg, gpu, d, size, halo, library="weno")
    for q in range(NTRACERS):
        assert not (new[q] == SENTINEL).all()
        _assert_parent(new[q], old[q], ("Nz = 1", q))


POISON = [((20, 12, 7), (3, 3, 1), F64), ((22, 6, 4), (3, 3, 1), F32), ((20, 11, 9), (4, 4, 4), F64), ((24, 11, 2), (4, 4, 4), F32),
          ((48, 40, 6), (5, 5, 5), F64), ((48, 40, 3), (5, 5, 5), F32), ((128, 5, 5), (3, 3, 1), F64), ((10, 10, 1), (4, 4, 4), F64)]


@pytest.mark.parametrize("case,offset", [(c, 0) for c in POISON] + [(OFFSET[1], 1)], ids=[_id(c) for c in POISON] + [_id(OFFSET[1]) + "-offset"])
def test_no_cell_outside_the_stencil_is_read(osg, gpu, case, offset):
    """every cell of the tracers, u, v, w and the metrics that cells_read does not list is NaN -- the z-halo planes beyond 0 and Nz + 1 at
    Hz = 4 and 5 among them: the result has no NaN and equals the clean one"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    read = cells_read(size, halo)
    assert Hz == 1 or (not read["c"][:Hz - 1].any() and not read["c"][Hz + Nz + 1:].any())
    poisoned = {k: np.where(read[k], h[k], dtype(np.nan)) for k in read if k != "c"}
    assert all(np.isnan(poisoned[k]).sum() == (~read[k]).sum() for k in poisoned) and all(np.isnan(poisoned[k]).any() for k in poisoned)
    poisoned["c"] = [np.where(read["c"], c, dtype(np.nan)) for c in h["c"]]
    assert all(np.isnan(c).sum() == (~read["c"]).sum() > 0 for c in poisoned["c"])
    poisoned["dz_c"] = h["dz_c"]
    got = _call(osg, gpu, _device(poisoned, gpu, offset), size, halo, offset=offset)
    for q in range(NTRACERS):
        assert not np.isnan(got[q]).any()
        _assert_parent(got[q], h["want"][q], ("poisoned", q))


@pytest.mark.parametrize("case", [((20, 12, 9), (3, 3, 1), F64), ((20, 12, 9), (3, 3, 1), F32), ((48, 40, 4), (5, 5, 5), F32)], ids=_id)
def test_selection_at_minus_zero_and_nan_of_mz(osg, gpu, case):
    """w with exact +0, -0 and NaN planted at faces of each order, in neighbouring columns of one chunk: -0 selects the left-biased value
    as +0 does, NaN the right-biased one (and makes the flux NaN) -- against the reference, and the selection against finite flows"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = dict(_case(case))
    w = h["w"].copy()
    k, j, i = np.indices(w.shape)
    sel = (i + 2 * j + k) % 4
    w[sel == 0] = 0.0
    w[sel == 1] = -0.0
    w[(i + j + 2 * k) % 7 == 3] = np.nan
    h["w"] = w
    orders = {face_order(f, Nz) for f in range(1, Nz + 2)}
    assert orders == ({2, 1, 3, 5} if Nz >= 6 else {2, 1, 3})
    for f in range(1, Nz + 2):                                     # every face has all three planted values in the interior
        plane = w[Hz + f - 1, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(plane).any() and (plane == 0).any() and np.signbit(plane[plane == 0]).any() and not np.signbit(plane[plane == 0]).all()
    want = [_ref(h, c, size, halo) for c in h["c"]]
    assert same_bits(want[0], h["want"][0]) > 0
    got = _call(osg, gpu, _device(h, gpu), size, halo)
    for q in range(NTRACERS):
        _assert_parent(got[q], want[q], ("planted w", q))
    # without an oracle: with u = v = 0, w = -0 everywhere gives what w = +0 everywhere gives -- zeros (the fluxes are zeros of the face
    # value's sign or its opposite, so G differs at most in the sign of a zero)
    h0, h1 = dict(_case(case)), dict(_case(case))
    h0["w"], h1["w"] = np.zeros_like(w), np.full_like(w, -0.0)
    h0["u"] = h1["u"] = np.zeros_like(h["u"])
    h0["v"] = h1["v"] = np.zeros_like(h["v"])
    g0, g1 = _call(osg, gpu, _device(h0, gpu), size, halo, which=(0,))[0], _call(osg, gpu, _device(h1, gpu), size, halo, which=(0,))[0]
    assert np.array_equal(g0, g1) and (g0[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] == 0).all()


SPECIAL = [((20, 12, 7), (3, 3, 1), F64), ((20, 12, 7), (3, 3, 1), F32), ((22, 6, 4), (3, 3, 1), F32), ((20, 11, 9), (4, 4, 4), F64),
           ((48, 40, 6), (5, 5, 5), F32), ((50, 40, 2), (4, 4, 4), F32)]


@pytest.mark.parametrize("case", SPECIAL, ids=_id)
def test_special_values_in_read_cells(osg, gpu, case):
    """+-0, subnormals, +-Inf, NaN, +-max (tests/special_values.pool) planted in 5 % of the cells of the tracers, u, v and w: bit for bit
    numpy's, which computes the same IEEE operations (Float32 subnormals included: the kernel flushes none)"""
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

    planted = {k: h[k] for k in SHARED}
    for name in ("u", "v", "w"):
        planted[name] = plant(h[name], 0.05)
    planted["c"] = [plant(c, 0.05) for c in h["c"]]
    c0 = planted["c"][0]                                           # whatever the draw gave: a NaN, an Inf, a -0 and a subnormal in one column
    c0[Hz, Hy + 1, Hx + 1], c0[Hz + Nz - 1, Hy + 1, Hx + 1], c0[Hz + 1, Hy + 2, Hx + 5], c0[Hz + 1, Hy + 4, Hx + 7] = np.nan, np.inf, -0.0, p[2]
    want = [_ref(planted, c, size, halo) for c in planted["c"]]
    inner = want[0][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert np.isnan(inner).any() and np.isfinite(inner).any()
    got = _call(osg, gpu, _device(planted, gpu), size, halo)
    for q in range(NTRACERS):
        _assert_parent(got[q], want[q], ("special values", q))
    # a tracer of subnormal magnitude throughout: the smoothness indicators underflow to 0 and the face values are subnormal
    tiny = np.finfo(dtype).tiny
    sub = dict(h)
    sub["c"] = [(c * tiny).astype(dtype) for c in h["c"][:1]]
    assert (np.abs(sub["c"][0]) < tiny).all() and (sub["c"][0] != 0).any()
    _assert_parent(_call(osg, gpu, _device(sub, gpu), size, halo)[0], _ref(sub, sub["c"][0], size, halo), "subnormal tracer")


MASKED = [((20, 12, 7), (3, 3, 1), F64), ((20, 12, 4), (3, 3, 1), F32), ((22, 6, 2), (3, 3, 1), F32), ((20, 11, 9), (4, 4, 4), F64),
          ((48, 40, 6), (5, 5, 5), F32), ((126, 5, 3), (4, 4, 4), F64), ((10, 10, 1), (4, 4, 4), F64)]


@pytest.mark.parametrize("case,offset", [(c, 0) for c in MASKED] + [(OFFSET[1], 1)], ids=[_id(c) for c in MASKED] + [_id(OFFSET[1]) + "-offset"])
def test_fused_mask_equals_the_reference(osg, gpu, case, offset):
    """with a count plane and a mask value that the type does not represent: the reference with the mask, on the whole parents.  Faces above
    the immersed bottom take the full order on the masked cells below them (the drop beside immersed nodes stays out)"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    n = _count_plane(case)
    want = [_ref(h, c, size, halo, n) for c in h["c"]]
    inner = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert (inner(want[0])[:, Ny - 1, Nx - 1] == dtype(MASK_VALUE)).all()                # n > Nz: the whole column
    assert same_bits(inner(want[0])[:, 0, 0], inner(h["want"][0])[:, 0, 0]) == 0         # n < 0: nothing
    assert same_bits(want[0], h["want"][0]) > 0
    got = _call(osg, gpu, _device(h, gpu, offset), size, halo, n_cc=_dev(n, gpu, offset), value=MASK_VALUE, offset=offset)
    for q in range(NTRACERS):
        _assert_parent(got[q], want[q], ("fused mask", q))


# ---- the domain of dependence in z: no oracle in the assertion ----------------------------------------------------------------------------
@pytest.mark.parametrize("positive", [True, False], ids=["w+", "w-"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_domain_of_dependence_in_z(osg, gpu, dtype, positive):
    """w of one sign, u = v = 0, Nz = 9 (the orders of the faces 1 .. 10: centred 1 3 5 5 5 5 3 1 centred): adding 1 to c at one cell of the
    level L moves G in that column exactly at the levels the order table allows (weno_xyz_ref.dependence_window, itself held to a
    hand-written list in tests/test_weno_xyz_ref.py) and in no other column -- for L = 1 (beside the wall), 2, 3, 5 (order 5 on both
    sides), 8 and 9.  One call per L with the bumped tracers as tracers 1 .. 6 beside the clean one; device results are compared with
    each other only"""
    case = ((20, 12, 9), (3, 3, 1), dtype)
    size, halo, _ = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = dict(_case(case))
    h["u"], h["v"] = np.zeros_like(h["u"]), np.zeros_like(h["v"])
    h["w"] = ((np.abs(h["w"]) + dtype(0.1)) * (1 if positive else -1)).astype(dtype)
    levels = (1, 2, 3, 5, 8, 9)
    j, i = 7, 13                                                   # 0-based interior cell: odd column, odd row -- mid-chunk, second row of a tile
    bumped = []
    for L in levels:
        c = h["c"][0].copy()
        c[Hz + L - 1, Hy + j, Hx + i] += 1
        bumped.append(c)
    h["c"] = [h["c"][0], *bumped]
    got = _call(osg, gpu, _device(h, gpu), size, halo)
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    for L, g in zip(levels, got[1:]):
        moved = cut(g) != cut(got[0])
        window = np.zeros((Nz, Ny, Nx), bool)
        window[:, j, i] = dependence_window(L, size, positive)
        assert np.array_equal(moved, window), (L, np.argwhere(moved != window)[:5])
    # by hand, level 5: the nodes 3 .. 7 whichever the sign; level 1 with w > 0: face 1 (centred), 2 (order 1, upwind cell 1), 3 (order 3:
    # 1, 2, 3), 4 (order 5: 1 .. 5) -> nodes 1 .. 4; with w < 0: face 1 (centred) only, face 2 takes cell 2 -> node 1
    assert np.flatnonzero(cut(got[4])[:, j, i] != cut(got[0])[:, j, i]).tolist() == [2, 3, 4, 5, 6]
    assert np.flatnonzero(cut(got[1])[:, j, i] != cut(got[0])[:, j, i]).tolist() == ([0, 1, 2, 3] if positive else [0])


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
DT, CHI = 0.01, 0.1


def _want(h, c, G0, size, halo):
    with np.errstate(all="ignore"):
        return tendency(c, h["u"], h["v"], h["w"], G0, h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo, h["n_cc"], 0.0)


@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 7), (5, 5, 5), torch.float64), ((50, 40, 6), (4, 4, 4), torch.float32)],
                         ids=["48x40x7-h5-f64", "50x40x6-h4-f32"])
def test_plan_eagerly_and_as_a_graph(osg, gpu, size, halo, tdt, immersed):
    """on a built TripolarGrid and on an ImmersedBoundaryGrid: the function (with each accepted scheme) and the plan give the reference's G on
    the filled fields (with the mask where there is one); the plan allocates nothing when called; tendency -> ab2_step_fields(fill_halos=True)
    twice eagerly and as one captured graph replayed twice from the same start give identical arrays"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, tracers, u, v, w, G, Gm = _model(osg, gpu, size, halo, tdt, immersed)
    h = _host_model(osg, grid, u, v, w)
    assert (h["n_cc"] is not None) == immersed
    want = [_want(h, c.data.cpu().numpy(), g.data.cpu().numpy(), size, halo) for c, g in zip(tracers, G)]
    tend = osg.weno_xyz_tracer_advection_plan(tracers, u, v, w, G)
    assert isinstance(tend, osg.WenoXyzTracerAdvectionPlan) and tend() is tend
    for q in range(len(tracers)):
        _assert_parent(G[q].data.cpu().numpy(), want[q], ("plan", q))
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    for scheme in (osg.WENO(), osg.WENO(order=5), osg.FluxFormAdvection(osg.WENO(), osg.WENO(), osg.WENO())):
        out = osg.weno_xyz_tracer_advection_tendency(tracers, u, v, w, scheme=scheme)
        for q in range(len(tracers)):
            assert out[q].grid is grid and out[q].loc == (osg.Center, osg.Center, osg.Center)
            bare = np.zeros_like(want[q])
            cut(bare)[...] = cut(want[q])
            _assert_parent(out[q].data.cpu().numpy(), bare, ("allocated", q))
    centred_in_z = osg.weno_tracer_advection_tendency(tracers, u, v, w)
    assert same_bits(centred_in_z[0].data.cpu().numpy(), out[0].data.cpu().numpy()) > 0          # not the existing call's rule
    # fill_halos: G's own conditions, on a copy of the interior the plan left
    filled = osg.weno_xyz_tracer_advection_tendency(tracers, u, v, w, out=[osg.CenterField(grid) for _ in tracers], fill_halos=True)
    for q in range(len(tracers)):
        twin = osg.CenterField(grid)
        twin.interior().copy_(G[q].interior())
        osg.fill_halo_regions([twin])
        _assert_parent(filled[q].data.cpu().numpy(), twin.data.cpu().numpy(), ("filled", q))
    # two steps eagerly, then one graph replayed twice from the same start
    step = osg.ab2_step_plan(tracers, G, Gm, DT, chi=CHI, fill_halos=True)
    everything = [*tracers, *G, *Gm]
    start = [f.data.clone() for f in everything]
    for _ in range(2):
        tend()
        step()
    eager = [f.data.clone() for f in everything]
    assert any(same_bits(a.cpu().numpy(), b.cpu().numpy()) > 0 for a, b in zip(start, eager))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    tend()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before              # the plan allocates nothing when called
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tend()
            step()
    torch.cuda.current_stream().wait_stream(side)
    for f, t in zip(everything, start):
        f.data.copy_(t)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for f, t in zip(everything, eager):
        _assert_parent(f.data.cpu().numpy(), t.cpu().numpy(), "two replays against two eager steps")


def test_seventeen_tracers_go_in_two_calls(osg, gpu):
    """17 tracers through the package: one call of 16 and one of 1"""
    size, halo, tdt = (20, 12, 6), (3, 3, 1), torch.float64
    grid, tracers, u, v, w, G, _ = _model(osg, gpu, size, halo, tdt, False, ntracers=17)
    h = _host_model(osg, grid, u, v, w)
    for g in G:
        g.data.fill_(SENTINEL)
    plan = osg.weno_xyz_tracer_advection_plan(tracers, u, v, w, G)
    assert plan() is plan and len(plan._before) == 1 and plan.tracers[16] is tracers[16]
    for q in range(17):
        c = tracers[q].data.cpu().numpy()
        _assert_parent(G[q].data.cpu().numpy(), _want(h, c, np.full(c.shape, SENTINEL, c.dtype), size, halo), ("17 tracers", q))


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched, the outputs keep the sentinel"""
    case = ((20, 12, 3), (3, 3, 1), F64)
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.weno_xyz_lib()
    err = lambda: lib.tpg_weno_xyz_last_error().decode()
    out = [_dev(np.full(h["c"][0].shape, SENTINEL, dtype), gpu) for _ in range(2)]
    assert _raw_call(osg, gpu, d, d["c"][:2], [out[0], d["c"][0]], size, halo) == -1 and err().startswith("G of tracer 1 overlaps tracer 0")
    # Hz = 0: the same arrays read as a geometry with no z-halo (3 + 2 levels fit the allocation of 5 planes)
    assert _raw_call(osg, gpu, d, d["c"][:2], out, (20, 12, 5), (3, 3, 0)) == -5
    assert err() == ("the rule reads c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1], u[i+1, j] and v[i, j+1]: "
                     "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (3,3,0))")
    with pytest.raises(osg._lib.TripolarHipError, match="TPG_ERR_UNSUPPORTED.*Hz >= 1 needed"):
        osg._lib.check_weno_xyz(_raw_call(osg, gpu, d, d["c"][:2], out, (20, 12, 5), (3, 3, 0)))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)


def test_example_two_forms_are_identical(osg, gpu):
    """examples/weno_xyz_tracer_step.py: tendency -> ab2_step_fields -> halo fill on a small immersed grid with 8 levels, eagerly and as one
    replayed graph, with identical bits"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("weno_xyz_tracer_step", os.path.join(root, "examples", "weno_xyz_tracer_step.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    eager, replayed = example.run(size=(60, 30, 8), steps=3, quiet=True)
    assert eager.keys() == replayed.keys() and len(eager) == 3
    for name in eager:
        a, b = eager[name].cpu().numpy(), replayed[name].cpu().numpy()
        assert np.isfinite(a).all()
        _assert_parent(a, b, ("example", name))
