"""GPU tests of the tracer advection tendency: tpg_tracer_advection_tendency through the C ABI, and tracer_advection_tendency /
tracer_advection_plan through the package.  Compared BIT FOR BIT with tests/advection_ref.py (numpy in the fields' type: every operation of the
rule is one correctly rounded IEEE operation, so the reference is exact and there is no tolerance anywhere in this file); NaNs compare by
NaN-ness; whole parents are compared: the halo cells of G against a sentinel, and the inputs must come back unchanged.

Shapes: the smallest at which each path can go wrong -- one level (both vertical faces read a halo plane); the minimum halo (every stencil
arm ends on the last halo cell); odd Hx (the element-aligned chunks), also with every pointer one element off the 16-B grid; more levels than
twice the look-ahead and no multiple of it; an odd Ny (a partial last row tile) on Float32 rows that sit on the 16-B grid; the model halo 5; Float32 with Nx = 2 mod 4 (8-B
chunks); one shape with more work items than are resident.  dz_c is random in [0.5, 2], so a wrong k index cannot hide."""
import ctypes as C

import numpy as np
import pytest
import torch

import ab2_ref
import gpu_harness as H
import tendency_windows as tw
from advection_ref import cells_read, interior_tendency, same_bits, tendency
from continuity_ref import w_and_divergence
from gpu_harness import (F32, F64, MASK_VALUE, SENTINEL, _assert_inputs_unchanged, _assert_parent, _count_plane, _dev, _filled,  # noqa: F401
                         _free_hbm, _id, _tracer_model as _model)
from special_values import pool

pytestmark = pytest.mark.gpu

KERNEL = tw.KERNELS["advection"]
#         size            halo       element type
SMALL = [((10, 10, 1), (4, 4, 4), F64),            # one level: both vertical faces read a halo plane
         ((20, 12, 3), (1, 1, 1), F64),            # every stencil arm ends on the last halo cell
         ((20, 12, 3), (1, 1, 1), F32),
         ((20, 12, 3), (3, 2, 1), F64),            # odd Hx: the element-aligned chunks
         ((20, 10, 9), (4, 4, 4), F64),            # more levels than twice the look-ahead (2) and no multiple of it
         ((24, 11, 5), (4, 4, 4), F32),            # Ny odd: the last row tile is a partial one (2 rows per item); Float32 rows on the 16-B grid
         ((48, 40, 6), (5, 5, 5), F64),            # the model halo
         ((48, 40, 6), (5, 5, 5), F32),
         ((50, 40, 3), (4, 4, 4), F32)]            # Nx = 2 mod 4: 8-B chunks
BIG = ((2304, 1283, 2), (4, 4, 4), F64)            # one tracer: >= 321 row tiles x 1152 chunks, more items than are resident; 1283 is odd
OFFSET = [SMALL[3], SMALL[4], SMALL[8]]            # every pointer one element off the 16-B grid: the GEN form by the pointers, not the rows
NTRACERS = 3


def _ref(h, c, size, halo, n_cc=None):
    """the reference parent of G of the tracer `c` from a sentinel-filled one; with a count plane: masked to MASK_VALUE"""
    return H._ref(KERNEL, h, size, halo, () if n_cc is None else (n_cc,), c)


def _case(case, ntracers=NTRACERS):
    return H._case(KERNEL, case, ntracers)


def _device(h, gpu, offset=0):
    return H._device(KERNEL, h, gpu, offset)


def _raw_call(osg, gpu, d, tracers, outs, size, halo, n_cc=None, value=0.0, scheme=0):
    return H._launch(osg, gpu, KERNEL, dict(d, c=tracers), {"G": outs}, size, halo, counts=(n_cc,), value=value, scheme=scheme)


def _call(osg, gpu, d, size, halo, which=None, n_cc=None, value=0.0, offset=0):
    """tpg_tracer_advection_tendency on the tracers `which` (indices; None: all) of the device arrays d into fresh sentinel-filled outputs ->
    the whole parents of G on the host"""
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
    """2304 x 1283 x 2, one tracer: 1152 chunks x at least 321 row tiles, several rounds of resident blocks; the last tile is a partial one"""
    size, halo, dtype = BIG
    h = _case(BIG, 1)
    d = _device(h, gpu)
    _assert_parent(_call(osg, gpu, d, size, halo)[0], h["want"][0], "big")
    _assert_parent(d["c"][0].cpu().numpy(), h["c"][0], "big: the tracer unchanged")


@pytest.mark.parametrize("case", [SMALL[4], SMALL[5]], ids=_id)
def test_sixteen_tracers_grouped_and_one_by_one(osg, gpu, case):
    """16 tracers in one call, against the reference and against sixteen calls of one tracer, calls of 5, 5, 5 and 1 and a call of 7, that one
    with a count plane too: identical bits however the call splits its tracers into groups"""
    size, halo, dtype = case
    h = _case(case, 16)
    d = _device(h, gpu)
    together = _call(osg, gpu, d, size, halo)
    assert len(together) == 16
    for q in range(16):
        _assert_parent(together[q], h["want"][q], ("16 tracers", q))
        _assert_parent(_call(osg, gpu, d, size, halo, which=(q,))[0], together[q], ("one by one", q))
    for q0 in (0, 5, 10, 15):
        part = _call(osg, gpu, d, size, halo, which=range(q0, min(q0 + 5, 16)))
        for q, got in enumerate(part, q0):
            _assert_parent(got, together[q], ("in fives", q))
    for q, got in enumerate(_call(osg, gpu, d, size, halo, which=range(3, 10)), 3):      # 7 = 4 + 2 + 1: every group size in one call
        _assert_parent(got, together[q], ("seven", q))
    n = _count_plane(case)
    masked = _call(osg, gpu, d, size, halo, which=range(3, 10), n_cc=_dev(n, gpu), value=MASK_VALUE)
    for q, got in enumerate(masked, 3):
        _assert_parent(got, _ref(h, h["c"][q], size, halo, n), ("seven, masked", q))
    _assert_inputs_unchanged(d, h, "16 tracers")


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[0], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[0]) + "-offset"])
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


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[0], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[0]) + "-offset"])
def test_fused_mask_equals_the_reference_and_the_mask_pass(osg, gpu, case, offset):
    """with a count plane: (1) the reference with the mask; (2) the unmasked call followed by tpg_mask_immersed_fields on G (zloc Center),
    bit for bit on the whole parents; without one nothing is masked (the first test)"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    n = _count_plane(case)
    want = [_ref(h, c, size, halo, n) for c in h["c"]]
    inner = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert (inner(want[0])[:, Ny - 1, Nx - 1] == dtype(MASK_VALUE)).all()                # n > Nz: the whole column
    assert same_bits(inner(want[0])[:, 0, 0], inner(h["want"][0])[:, 0, 0]) == 0         # n < 0: nothing
    assert same_bits(want[0], h["want"][0]) > 0
    d = _device(h, gpu, offset)
    nd = _dev(n, gpu, offset)
    got = _call(osg, gpu, d, size, halo, n_cc=nd, value=MASK_VALUE, offset=offset)
    for q in range(NTRACERS):
        _assert_parent(got[q], want[q], ("fused mask", q))
    # the two-pass form, on what the unmasked call leaves (held equal to h["want"] by the first test)
    lib = osg._lib.lib()
    for q in range(NTRACERS):
        t = _dev(h["want"][q], gpu, offset)
        osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table([t]), 1, osg._lib.ptr_table([nd]), (C.c_int8 * 1)(osg._lib.TPG_CENTER),
                                                    (C.c_double * 1)(MASK_VALUE), Nx, Ny, Nz, *halo, osg._lib.ft_of(t.dtype),
                                                    osg._lib.current_stream_ptr(gpu)))
        _assert_parent(t.cpu().numpy(), want[q], ("two passes", q))


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[0], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[0]) + "-offset"])
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max planted in 5 % of the cells of the tracers, u, v and w and 3 % of each metric plane (az_cc = +-0
    among them: 1 / 0): bit for bit numpy's, which computes the same IEEE operations"""
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

    planted = {"dz_c": h["dz_c"]}
    for name, share in (("u", 0.05), ("v", 0.05), ("w", 0.05), ("dy_fc", 0.03), ("dx_cf", 0.03), ("az_cc", 0.03)):
        planted[name] = plant(h[name], share)
    planted["c"] = [plant(c, 0.05) for c in h["c"]]
    # whatever the draw gave the small shapes: a zero area of either sign, a NaN, an Inf and a -0 tracer cell in the interior
    planted["az_cc"][Hy, Hx], planted["az_cc"][Hy + Ny - 1, Hx + Nx - 1] = 0.0, -0.0
    planted["c"][0][Hz, Hy + 1, Hx + 1], planted["c"][0][Hz, Hy + 3, Hx + 3], planted["c"][0][Hz, Hy + 5, Hx + 5] = np.nan, np.inf, -0.0
    want = [_ref(planted, c, size, halo) for c in planted["c"]]
    inner = want[0][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert np.isnan(inner).any() and np.isinf(inner).any() and np.isfinite(inner).mean() > 0.3
    got = _call(osg, gpu, _device(planted, gpu, offset), size, halo, offset=offset)
    for q in range(NTRACERS):
        _assert_parent(got[q], want[q], ("special values", q))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_signs_of_zero(osg, gpu, dtype):
    """c = 0 everywhere: every flux is +-0 and the rule's leading minus is a sign flip of the zero the sums leave -- the bits numpy gives"""
    case = ((20, 12, 3), (1, 1, 1), dtype)
    size, halo, _ = case
    h = dict(_case(case))
    h["c"] = [np.zeros_like(h["c"][0]), -np.zeros_like(h["c"][0])]
    want = [_ref(h, c, size, halo) for c in h["c"]]
    assert (want[0][1:-1, 1:-1, 1:-1] == 0).all() and np.signbit(want[0][1:-1, 1:-1, 1:-1]).any()
    got = _call(osg, gpu, _device(h, gpu), size, halo)
    for q in range(2):
        _assert_parent(got[q], want[q], ("zeros", q))


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched, the outputs keep the sentinel"""
    case = SMALL[1]
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.advection_lib()
    err = lambda: lib.tpg_advection_last_error().decode()
    out = [_dev(np.full(h["c"][0].shape, SENTINEL, dtype), gpu) for _ in range(2)]
    assert _raw_call(osg, gpu, d, d["c"][:2], [out[0], d["c"][0]], size, halo) == -1 and err().startswith("G of tracer 1 overlaps tracer 0")
    assert _raw_call(osg, gpu, d, d["c"][:2], [d["w"], out[1]], size, halo) == -1 and err().startswith("G of tracer 0 overlaps w")
    assert _raw_call(osg, gpu, d, d["c"][:2], out, size, halo, scheme=2) == -5 and "scheme 2 is not built" in err()
    # Hz = 0: the same arrays read as a geometry without a vertical halo (3 + 2 levels x 14 x 22 cells fit the allocation)
    assert _raw_call(osg, gpu, d, d["c"][:2], out, (20, 12, 5), (1, 1, 0)) == -5 and "Hz >= 1 needed (halo (1,1,0))" in err()
    with pytest.raises(osg._lib.TripolarHipError, match="TPG_ERR_UNSUPPORTED.*Hz >= 1 needed"):
        osg._lib.check_advection(_raw_call(osg, gpu, d, d["c"][:2], out, (20, 12, 5), (1, 1, 0)))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)
    _assert_inputs_unchanged(d, h, "refusals")


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
DT, CHI = 0.01, 0.1


def _host_model(osg, grid, u, v, w, size, halo):
    """the harness's host model, its w held equal to the continuity reference's"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = H._host_model(osg, grid, u, v, w)
    want_w, _ = w_and_divergence(h["u"], h["v"], np.zeros_like(h["w"]), None, h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo, h["n_cc"], 0.0)
    cut = (slice(Hz, Hz + Nz + 1), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    _assert_parent(h["w"][cut], want_w[cut], "w is the continuity reference's")
    return h


@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)],
                         ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_two_steps_eagerly_and_as_a_graph_equal_the_references_composed(osg, gpu, size, halo, tdt, immersed):
    """filled c, u, v, w from compute_w_from_continuity, then twice: tendency -> ab2_step_fields(fill_halos=True).  Eagerly, every G, c and
    Gm after each step is the composition of advection_ref, ab2_ref and the fill's; one captured graph of the two plans replayed twice from
    the start gives the same arrays.  On the immersed grid the mask in the call is mask_immersed_field on G"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, tracers, u, v, w, G, Gm = _model(osg, gpu, size, halo, tdt, immersed)
    h = _host_model(osg, grid, u, v, w, size, halo)
    assert (h["n_cc"] is not None) == immersed
    tend = osg.tracer_advection_plan(tracers, u, v, w, G)
    step = osg.ab2_step_plan(tracers, G, Gm, DT, chi=CHI, fill_halos=True)
    everything = [*tracers, *G, *Gm]
    start = [f.data.clone() for f in everything]
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    host = [[f.data.cpu().numpy() for f in fs] for fs in (tracers, G, Gm)]
    for it in range(2):
        assert tend() is tend and step() is step
        for q in range(len(tracers)):
            c0, G0, Gm0 = (host[s][q] for s in range(3))
            with np.errstate(all="ignore"):
                want_G = tendency(c0, h["u"], h["v"], h["w"], G0, h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo, h["n_cc"], 0.0)
            new, prev, _ = ab2_ref.ab2_step(c0, want_G, Gm0, DT, CHI, ab2_ref.STORE, size, halo)
            new = _filled(osg, tracers[q], cut(new), c0)
            _assert_parent(G[q].data.cpu().numpy(), want_G, ("G", it, q))
            _assert_parent(tracers[q].data.cpu().numpy(), new, ("tracer", it, q))
            _assert_parent(Gm[q].data.cpu().numpy(), prev, ("Gm", it, q))
            assert same_bits(cut(new), cut(c0)) > 0 and same_bits(cut(want_G), cut(G0)) > 0      # the step and the tendency changed something
            host[0][q], host[1][q], host[2][q] = new, want_G, prev
    eager = [f.data.clone() for f in everything]
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
    if immersed:                                                   # the mask value of the call is the mask pass's
        raw = osg.tracer_advection_tendency(tracers, u, v, w, mask_immersed=False)
        masked = osg.tracer_advection_tendency(tracers, u, v, w)
        assert all(same_bits(a.data.cpu().numpy(), b.data.cpu().numpy()) > 0 for a, b in zip(raw, masked))
        osg.mask_immersed_field(raw, 0)
        for q, (a, b) in enumerate(zip(raw, masked)):
            _assert_parent(a.data.cpu().numpy(), b.data.cpu().numpy(), ("mask pass", q))


def test_seventeen_tracers_go_in_two_calls_and_out_is_allocated(osg, gpu):
    """17 tracers through the package: one call of 16 and one of 1; `out=None` allocates CenterFields whose halos stay zero; fill_halos fills
    the tendencies' own halos"""
    size, halo, tdt = (20, 12, 3), (3, 2, 1), torch.float64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, tracers, u, v, w, G, _ = _model(osg, gpu, size, halo, tdt, False, ntracers=17)
    h = _host_model(osg, grid, u, v, w, size, halo)
    for g in G:
        g.data.fill_(SENTINEL)
    plan = osg.tracer_advection_plan(tracers, u, v, w, G)
    assert plan() is plan and len(plan._before) == 1 and plan.G is not None and plan.tracers[16] is tracers[16]
    want = []
    for q in range(17):
        c = tracers[q].data.cpu().numpy()
        want.append(tendency(c, h["u"], h["v"], h["w"], np.full(c.shape, SENTINEL, c.dtype), h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo))
        _assert_parent(G[q].data.cpu().numpy(), want[q], ("17 tracers", q))
    out = osg.tracer_advection_tendency(tracers[:2], u, v, w)
    assert len(out) == 2 and all(o.loc == (osg.Center, osg.Center, osg.Center) and o.grid is grid for o in out)
    for q in range(2):
        bare = np.zeros_like(want[q])
        bare[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = want[q][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        _assert_parent(out[q].data.cpu().numpy(), bare, ("allocated", q))
    given = osg.tracer_advection_tendency(tracers[:2], u, v, w, out=G[:2], fill_halos=True)
    assert given[0] is G[0] and given[1] is G[1]
    for q in range(2):
        _assert_parent(G[q].data.cpu().numpy(), _filled(osg, G[q], want[q][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], want[q]), ("filled", q))
    _assert_parent(interior_tendency(tracers[0].data.cpu().numpy(), h["u"], h["v"], h["w"], h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo),
                   out[0].interior().cpu().numpy(), "interior")          # of the unfilled field: the fold rewrites half of a Center field's row Ny
