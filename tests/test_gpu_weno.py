"""GPU tests of the WENO5 tracer advection tendency: tpg_weno_tracer_advection_tendency through the C ABI, and
weno_tracer_advection_tendency / weno_tracer_advection_plan through the package.  Compared BIT FOR BIT with tests/weno_ref.py (numpy in the
fields' type: every operation of the rule is one correctly rounded IEEE operation, so the reference is exact and there is no tolerance
anywhere in this file); NaNs compare by NaN-ness; whole parents are compared: the halo cells of G against a sentinel, and the inputs must
come back unchanged.

Shapes: the smallest at which each path can go wrong -- one level (both vertical faces read a halo plane); the minimum halo (3, 3, 1)
(every stencil arm ends on the last halo cell; in Float32 with 16-B chunks the chunk past a row's end would leave the halo, so the kernel
takes its plain form, with 8-B chunks its flux-sharing form with the clamped east reads); more levels than a ring of look-ahead slots
holds, an odd Ny (a partial last row tile); Float32 rows on the 16-B grid; the model halo 5 (element-aligned chunks), also with every
pointer one element off the 16-B grid; Float32 with Nx = 2 mod 4 (8-B chunks); rows of exactly 63 chunks and of 64 (a wave of the
flux-sharing form stores 63: the chunk past the row's end is the wave's last lane, or the second lane of a wave of its own); one shape with
more work items than are resident.  dz_c and the metrics are random in [0.5, 2], u, v, w of both signs."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import gpu_harness as H
import tendency_windows as tw
from gpu_harness import (F32, F64, MASK_VALUE, SENTINEL, _assert_inputs_unchanged, _assert_parent, _count_plane, _dev, _free_hbm, _host_model,  # noqa: F401
                         _id, _tracer_model as _model)
from special_values import pool
from weno_ref import cells_read, dependence_window, interior_tendency, same_bits, tendency

pytestmark = pytest.mark.gpu

KERNEL = tw.KERNELS["weno"]
#         size            halo       element type
SMALL = [((10, 10, 1), (4, 4, 4), F64),            # one level: both vertical faces read a halo plane
         ((20, 12, 3), (3, 3, 1), F64),            # every stencil arm ends on the last halo cell
         ((20, 12, 3), (3, 3, 1), F32),            # 16-B chunks wider than Hx: the plain form
         ((22, 6, 2), (3, 3, 1), F32),             # 8-B chunks, Hx = 3: the chunk past the row's end fills the halo, its east reads are clamped
         ((20, 11, 9), (4, 4, 4), F64),            # nine levels, Ny odd: the last row tile is a partial one
         ((24, 11, 5), (4, 4, 4), F32),            # the same on Float32 rows that sit on the 16-B grid
         ((48, 40, 6), (5, 5, 5), F64),            # the model halo: the element-aligned chunks
         ((48, 40, 6), (5, 5, 5), F32),
         ((50, 40, 3), (4, 4, 4), F32),            # Nx = 2 mod 4: 8-B chunks
         ((126, 5, 2), (4, 4, 4), F64),            # 63 chunks a row: one full wave, its last lane the chunk past the end
         ((128, 5, 2), (3, 3, 1), F64),            # 64 chunks a row: the last chunk and the one past the end in a wave of their own
         ((252, 5, 2), (4, 4, 4), F32)]            # 63 chunks of 16 B
# One tracer, Float64: 1152 chunks a row = 19 waves (63 chunks each) x 322 row tiles (2 rows each) = 6118 waves.  The kernel takes 214 - 226
# VGPRs, so 2 waves per SIMD: 256 CUs x 4 SIMDs x 2 = 2048 waves are resident -- three rounds.  643 is odd: the last tile is a partial one.
BIG = ((2304, 643, 2), (4, 4, 4), F64)
OFFSET = [SMALL[4], SMALL[6], SMALL[8]]            # every pointer one element off the 16-B grid: the GEN form by the pointers, not the rows
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


def _call(osg, gpu, d, size, halo, which=None, n_cc=None, value=0.0, offset=0):
    """tpg_weno_tracer_advection_tendency on the tracers `which` (indices; None: all) of the device arrays d into fresh sentinel-filled
    outputs -> the whole parents of G on the host"""
    return H._call(osg, gpu, KERNEL, d, size, halo, which, (n_cc,), value, offset)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(c, 1) for c in OFFSET],
                         ids=[_id(c) for c in SMALL] + [_id(c) + "-offset" for c in OFFSET])
def test_interior_is_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, offset):
    """random data in every cell, the parents of G pre-filled with a sentinel: with 1, 2 and 3 tracers in a call the whole parents equal the
    reference's -- the interior the rule, every halo cell still the sentinel -- and every input comes back as it was"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    for want in h["want"]:                                         # the reference parents themselves: sentinel exactly on the halo cells
        edge = np.ones(want.shape, bool)
        edge[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
        assert (want[edge] == SENTINEL).all() and not (want[~edge] == SENTINEL).any() and np.isfinite(want).all()
    assert same_bits(h["want"][0], h["want"][1]) > 0.9 * Nx * Ny * Nz
    d = _device(h, gpu, offset)
    for n in (1, 2, 3):
        got = _call(osg, gpu, d, size, halo, which=range(n), offset=offset)
        for q in range(n):
            _assert_parent(got[q], h["want"][q], ("parent", n, q))
    got = _call(osg, gpu, d, size, halo, which=(2, 0), offset=offset)                    # the order of the table is the caller's
    _assert_parent(got[0], h["want"][2], "reordered 2")
    _assert_parent(got[1], h["want"][0], "reordered 0")
    _assert_inputs_unchanged(d, h, "parent")


def test_more_items_than_are_resident(osg, gpu):
    """2304 x 643 x 2, one tracer: several rounds of resident waves (the arithmetic is at BIG); the last tile is a partial one"""
    size, halo, dtype = BIG
    h = _case(BIG, 1)
    d = _device(h, gpu)
    _assert_parent(_call(osg, gpu, d, size, halo)[0], h["want"][0], "big")
    _assert_parent(d["c"][0].cpu().numpy(), h["c"][0], "big: the tracer unchanged")


@pytest.mark.parametrize("case", [SMALL[4], SMALL[5]], ids=_id)
def test_seven_tracers_grouped_and_one_by_one(osg, gpu, case):
    """7 tracers in one call (4 + 2 + 1 where the build groups them), against the reference and against seven calls of one tracer and calls
    of 3, 3 and 1, and with a count plane too: identical bits however the call splits its tracers into groups"""
    size, halo, dtype = case
    h = _case(case, 7)
    d = _device(h, gpu)
    together = _call(osg, gpu, d, size, halo)
    assert len(together) == 7
    for q in range(7):
        _assert_parent(together[q], h["want"][q], ("7 tracers", q))
        _assert_parent(_call(osg, gpu, d, size, halo, which=(q,))[0], together[q], ("one by one", q))
    for q0 in (0, 3, 6):
        part = _call(osg, gpu, d, size, halo, which=range(q0, min(q0 + 3, 7)))
        for q, got in enumerate(part, q0):
            _assert_parent(got, together[q], ("in threes", q))
    n = _count_plane(case)
    masked = _call(osg, gpu, d, size, halo, n_cc=_dev(n, gpu), value=MASK_VALUE)
    for q, got in enumerate(masked):
        _assert_parent(got, _ref(h, h["c"][q], size, halo, n), ("seven, masked", q))
    _assert_inputs_unchanged(d, h, "7 tracers")


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[1], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[1]) + "-offset"])
def test_no_cell_outside_the_stencil_is_read(osg, gpu, case, offset):
    """every cell of the tracers, u, v, w and the metrics that the rule does not read is NaN: the result has no NaN and equals the clean one"""
    size, halo, dtype = case
    h = _case(case)
    read = cells_read(size, halo)
    poisoned = {k: np.where(read[k], h[k], dtype(np.nan)) for k in read if k != "c"}
    assert all(np.isnan(poisoned[k]).sum() == (~read[k]).sum() for k in poisoned) and all(np.isnan(poisoned[k]).any() for k in poisoned)
    poisoned["c"] = [np.where(read["c"], c, dtype(np.nan)) for c in h["c"]]
    assert all(np.isnan(c).sum() == (~read["c"]).sum() > 0 for c in poisoned["c"])
    poisoned["dz_c"] = h["dz_c"]
    got = _call(osg, gpu, _device(poisoned, gpu, offset), size, halo, offset=offset)
    for q in range(NTRACERS):
        assert not np.isnan(got[q]).any()
        _assert_parent(got[q], h["want"][q], ("poisoned", q))


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[1], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[1]) + "-offset"])
def test_fused_mask_equals_the_reference(osg, gpu, case, offset):
    """with a count plane and a mask value that the type does not represent: the reference with the mask, on the whole parents; without one
    nothing is masked (the first test)"""
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


@pytest.mark.parametrize("case", [SMALL[1], SMALL[2], SMALL[3], SMALL[7]], ids=_id)
def test_sign_selection_inside_one_chunk(osg, gpu, case):
    """u and v alternate in sign from cell to cell, with exact +0 and -0 planted every third cell: inside every chunk and every row tile the
    faces select different sides (+0 and -0 the left-biased one) -- five selects, no branch to get wrong"""
    size, halo, dtype = case
    h = dict(_case(case))
    k, j, i = np.indices(h["u"].shape)
    flip = np.where((i + j + k) % 2 == 0, dtype(1), dtype(-1))
    for name in ("u", "v"):
        a = np.abs(h[name]) * flip
        a[(i + 2 * j + k) % 3 == 0] = 0.0
        a[(i + 2 * j + k) % 6 == 3] = -0.0
        h[name] = a.astype(dtype)
    assert (h["u"] == 0).any() and np.signbit(h["u"][h["u"] == 0]).any() and not np.signbit(h["u"][h["u"] == 0]).all()
    want = [_ref(h, c, size, halo) for c in h["c"]]
    assert same_bits(want[0], h["want"][0]) > 0
    got = _call(osg, gpu, _device(h, gpu), size, halo)
    for q in range(NTRACERS):
        _assert_parent(got[q], want[q], ("signs", q))


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL[:9]] + [(OFFSET[1], 1)],
                         ids=[_id(c) for c in SMALL[:9]] + [_id(OFFSET[1]) + "-offset"])
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max (tests/special_values.pool) planted in 5 % of the cells of the tracers, u and v: bit for bit
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
    for name in ("u", "v"):
        planted[name] = plant(h[name], 0.05)
    planted["c"] = [plant(c, 0.05) for c in h["c"]]
    # whatever the draw gave the small shapes: a NaN, an Inf, a -0 and a subnormal tracer cell in the interior, a NaN and a -0 velocity
    c0 = planted["c"][0]
    c0[Hz, Hy + 1, Hx + 1], c0[Hz, Hy + 3, Hx + 3], c0[Hz, Hy + 2, Hx + 5], c0[Hz, Hy + 4, Hx + 7] = np.nan, np.inf, -0.0, p[2]
    planted["u"][Hz, Hy + 2, Hx + 2], planted["v"][Hz, Hy + 2, Hx + 8] = np.nan, -0.0
    want = [_ref(planted, c, size, halo) for c in planted["c"]]
    inner = want[0][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert np.isnan(inner).any() and np.isfinite(inner).any()
    got = _call(osg, gpu, _device(planted, gpu, offset), size, halo, offset=offset)
    for q in range(NTRACERS):
        _assert_parent(got[q], want[q], ("special values", q))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_subnormal_tracer(osg, gpu, dtype):
    """a tracer of subnormal magnitude throughout: the smoothness indicators underflow to 0, tau / eps is 0, the weights are the linear
    ones and the face values are subnormal -- bit for bit numpy's"""
    case = ((20, 12, 3), (3, 3, 1), dtype)
    size, halo, _ = case
    h = dict(_case(case))
    tiny = np.finfo(dtype).tiny
    h["c"] = [(c * tiny).astype(dtype) for c in h["c"][:2]]
    assert all((np.abs(c) < tiny).all() and (c != 0).any() for c in h["c"])
    want = [_ref(h, c, size, halo) for c in h["c"]]
    got = _call(osg, gpu, _device(h, gpu), size, halo)
    for q in range(2):
        _assert_parent(got[q], want[q], ("subnormal tracer", q))


# ---- the domain of dependence: no oracle in the assertion ---------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,positive", [("x", True), ("x", False), ("y", True), ("y", False)], ids=["u+", "u-", "v+", "v-"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_domain_of_dependence(osg, gpu, dtype, axis, positive):
    """one-signed flow along one axis, the other velocities zero: adding 1 to c at one interior cell n* changes G nowhere outside
    n* - 2 .. n* + 3 (flow > 0; n* - 3 .. n* + 2 for flow < 0) of that row (column) and level, and does change it at n* + 3 (n* - 3).
    Confirmed on weno_ref first (also tests/test_weno_ref.py); the device results are compared with each other only"""
    case = ((48, 40, 6), (5, 5, 5), dtype)
    size, halo, _ = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = dict(_case(case))
    flow = (np.abs(h["u" if axis == "x" else "v"]) + dtype(0.1)).astype(dtype)
    h["u"], h["v"], h["w"] = np.zeros_like(h["u"]), np.zeros_like(h["v"]), np.zeros_like(h["w"])
    h["u" if axis == "x" else "v"] = flow if positive else -flow
    k, j, i = 2, 17, 21                                            # 0-based interior cell: odd column, odd row -- mid-chunk, second row of a tile
    c1 = h["c"][0].copy()
    c1[Hz + k, Hy + j, Hx + i] += 1
    h["c"] = [h["c"][0], c1]
    lo, hi = (-2, 3) if positive else (-3, 2)
    window = np.zeros((Nz, Ny, Nx), bool)
    if axis == "x":
        window[k, j, i + lo:i + hi + 1] = True
        far = (k, j, i + (3 if positive else -3))
    else:
        window[k, j + lo:j + hi + 1, i] = True
        far = (k, j + (3 if positive else -3), i)
    assert np.array_equal(window, dependence_window(h["c"][1] != h["c"][0], size, halo, axis, positive))
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    ref_moved = cut(_ref(h, h["c"][0], size, halo)) != cut(_ref(h, h["c"][1], size, halo))
    assert ref_moved[far] and not (ref_moved & ~window).any()      # the reference first
    base, bumped = _call(osg, gpu, _device(h, gpu), size, halo)
    moved = cut(base) != cut(bumped)
    assert moved[far], "the far end of the upwind stencil is not read"
    assert not (moved & ~window).any(), np.argwhere(moved & ~window)[:5]


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
DT, CHI = 0.01, 0.1


def _want(h, c, G0, size, halo, masked=True):
    with np.errstate(all="ignore"):
        return tendency(c, h["u"], h["v"], h["w"], G0, h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo, h["n_cc"] if masked else None, 0.0)


@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)],
                         ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_plan_eagerly_and_as_a_graph(osg, gpu, size, halo, tdt, immersed):
    """on a built TripolarGrid and on an ImmersedBoundaryGrid: the function and the plan give the reference's G on the filled fields (with
    the mask where there is one); the plan allocates nothing when called; tendency -> ab2_step_fields(fill_halos=True) twice eagerly and as
    one captured graph replayed twice from the same start give identical arrays; fill_halos fills G's own halos"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, tracers, u, v, w, G, Gm = _model(osg, gpu, size, halo, tdt, immersed)
    h = _host_model(osg, grid, u, v, w)
    assert (h["n_cc"] is not None) == immersed
    want = [_want(h, c.data.cpu().numpy(), g.data.cpu().numpy(), size, halo) for c, g in zip(tracers, G)]
    tend = osg.weno_tracer_advection_plan(tracers, u, v, w, G)
    assert isinstance(tend, osg.WenoTracerAdvectionPlan) and tend() is tend
    for q in range(len(tracers)):
        _assert_parent(G[q].data.cpu().numpy(), want[q], ("plan", q))
    out = osg.weno_tracer_advection_tendency(tracers, u, v, w, scheme=osg.FluxFormAdvection(osg.WENO(), osg.WENO(order=5), osg.Centered()))
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    for q in range(len(tracers)):
        assert out[q].grid is grid and out[q].loc == (osg.Center, osg.Center, osg.Center)
        bare = np.zeros_like(want[q])
        cut(bare)[...] = cut(want[q])
        _assert_parent(out[q].data.cpu().numpy(), bare, ("allocated", q))
    if immersed:
        raw = osg.weno_tracer_advection_tendency(tracers, u, v, w, mask_immersed=False)
        for q in range(len(tracers)):
            _assert_parent(cut(raw[q].data.cpu().numpy()), cut(_want(h, tracers[q].data.cpu().numpy(), want[q], size, halo, masked=False)), ("unmasked", q))
        assert any(same_bits(a.data.cpu().numpy(), b.data.cpu().numpy()) > 0 for a, b in zip(raw, out))
    # fill_halos: G's own conditions, on a copy of the interior the plan left
    filled = osg.weno_tracer_advection_tendency(tracers, u, v, w, out=[osg.CenterField(grid) for _ in tracers], fill_halos=True)
    for q in range(len(tracers)):
        twin = osg.CenterField(grid)
        twin.interior().copy_(G[q].interior())
        osg.fill_halo_regions([twin])
        _assert_parent(filled[q].data.cpu().numpy(), twin.data.cpu().numpy(), ("filled", q))
        assert same_bits(filled[q].data.cpu().numpy(), out[q].data.cpu().numpy()) > 0
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


@pytest.mark.parametrize("where", ["seam", "zipper"])
def test_dependence_across_the_seam_and_into_the_zipper_halo(osg, gpu, where):
    """through the package, halos filled: with u > 0 a bump two cells west of the periodic seam reaches the first columns of its row; with
    v > 0 a bump in row Ny - 1 reaches row Ny and, through the Zipper's halo rows, whatever interior nodes read the folded image -- and no
    node outside the windows of the cells the fill changed"""
    size, halo, tdt = (48, 40, 3), (5, 5, 5), torch.float64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, tracers, u, v, w, G, _ = _model(osg, gpu, size, halo, tdt, False, ntracers=1)
    axis = "x" if where == "seam" else "y"
    flow, still = (u, v) if axis == "x" else (v, u)
    flow.data.copy_(flow.data.abs() + 0.1)
    still.data.zero_()
    w.data.zero_()
    c = tracers[0]
    k, j, i = (1, 8, Nx - 2) if where == "seam" else (1, Ny - 2, 13)
    base_c = c.data.cpu().numpy()
    base = osg.weno_tracer_advection_tendency([c], u, v, w)[0].interior().cpu().numpy()
    c.data[Hz + k, Hy + j, Hx + i] += 1
    osg.fill_halo_regions([c])
    changed = c.data.cpu().numpy() != base_c
    assert changed.sum() > 1                                       # the fill carried the bump into a halo
    bumped = osg.weno_tracer_advection_tendency([c], u, v, w)[0].interior().cpu().numpy()
    moved = base != bumped
    window = dependence_window(changed, size, halo, axis, True)
    h = _host_model(osg, grid, u, v, w)
    ref_moved = (interior_tendency(base_c, h["u"], h["v"], h["w"], h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo)
                 != interior_tendency(c.data.cpu().numpy(), h["u"], h["v"], h["w"], h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo))
    if where == "seam":
        far = (k, j, 1)                                            # i* + 3 is one past the seam's first column: it reads the bump in the west halo
        assert window[k, j, 0] and window[k, j, 1] and not window[k, j, 2]
    else:
        far = (k, Ny - 1, i)                                       # row Ny reads the bump directly; rows beyond are the fold's
        assert window[k, Ny - 1, i] and window.sum() > 4
    assert ref_moved[far] and not (ref_moved & ~window).any()      # the reference first
    assert moved[far]
    assert not (moved & ~window).any(), np.argwhere(moved & ~window)[:5]
    assert np.array_equal(moved, ref_moved)


def test_seventeen_tracers_go_in_two_calls(osg, gpu):
    """17 tracers through the package: one call of 16 and one of 1"""
    size, halo, tdt = (20, 12, 3), (3, 3, 1), torch.float64
    grid, tracers, u, v, w, G, _ = _model(osg, gpu, size, halo, tdt, False, ntracers=17)
    h = _host_model(osg, grid, u, v, w)
    for g in G:
        g.data.fill_(SENTINEL)
    plan = osg.weno_tracer_advection_plan(tracers, u, v, w, G)
    assert plan() is plan and len(plan._before) == 1 and plan.tracers[16] is tracers[16]
    for q in range(17):
        c = tracers[q].data.cpu().numpy()
        _assert_parent(G[q].data.cpu().numpy(), _want(h, c, np.full(c.shape, SENTINEL, c.dtype), size, halo), ("17 tracers", q))


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched, the outputs keep the sentinel"""
    case = SMALL[1]
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.weno_lib()
    err = lambda: lib.tpg_weno_last_error().decode()
    out = [_dev(np.full(h["c"][0].shape, SENTINEL, dtype), gpu) for _ in range(2)]
    assert _raw_call(osg, gpu, d, d["c"][:2], [out[0], d["c"][0]], size, halo) == -1 and err().startswith("G of tracer 1 overlaps tracer 0")
    assert _raw_call(osg, gpu, d, d["c"][:2], [d["w"], out[1]], size, halo) == -1 and err().startswith("G of tracer 0 overlaps w")
    # Hx = 2: the same arrays read as a geometry with a narrower halo (22 + 4 columns x 14 + 4 rows fit the allocation of 26 x 18)
    assert _raw_call(osg, gpu, d, d["c"][:2], out, (22, 12, 3), (2, 3, 1)) == -5 and "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,3,1))" in err()
    with pytest.raises(osg._lib.TripolarHipError, match="TPG_ERR_UNSUPPORTED.*Hz >= 1 needed"):
        osg._lib.check_weno(_raw_call(osg, gpu, d, d["c"][:2], out, (22, 12, 3), (2, 3, 1)))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)
    _assert_inputs_unchanged(d, h, "refusals")


def test_example_two_forms_are_identical(osg, gpu):
    """examples/weno_tracer_step.py: tendency -> ab2_step_fields -> halo fill on a small immersed grid, eagerly and as one replayed graph,
    with identical bits"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("weno_tracer_step", os.path.join(root, "examples", "weno_tracer_step.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    eager, replayed = example.run(size=(60, 30, 3), steps=3, quiet=True)
    assert eager.keys() == replayed.keys() and len(eager) == 3
    for name in eager:
        a, b = eager[name].cpu().numpy(), replayed[name].cpu().numpy()
        assert np.isfinite(a).all()
        _assert_parent(a, b, ("example", name))
