"""GPU tests of the momentum advection tendency: tpg_momentum_advection_tendency through the C ABI, and momentum_advection_tendency /
momentum_advection_plan through the package.  Compared BIT FOR BIT with tests/momentum_ref.py (numpy in the fields' type: every operation of
the rule is one correctly rounded IEEE operation, so the reference is exact and there is no tolerance anywhere in this file); NaNs compare by
NaN-ness; whole parents are compared: the halo cells of Gu, Gv against a sentinel, and the inputs must come back unchanged.

Shapes: the tracer tendency's list, the smallest at which each path can go wrong -- one level (both vertical faces read a halo plane); the
minimum halo (every stencil arm and both corners end on the last halo cell); odd Hx (the element-aligned chunks), also with every pointer one
element off the 16-B grid; more levels than twice the look-ahead and no multiple of it; an odd Ny (a partial last row tile) on Float32
rows that sit on the 16-B grid; the model halo 5; Float32 with Nx = 2 mod 4 (8-B chunks); one shape with more work items than are
resident.  The committed kernel takes 1 row per item and look-ahead 1 in Float64, 2 rows and look-ahead 2 in Float32, so the list needs no
further size: the partial tile exists in Float32 only and 24 x 11 x 5 is a Float32 case, whose 5 levels are also more than twice that
look-ahead and no multiple of it (9 levels do the same for Float64, and for its measured 2-row / look-ahead-2 variants 10 rows stay whole).
dz_f is random in [0.5, 2], so a wrong face index cannot hide."""
import ctypes as C

import numpy as np
import pytest
import torch

import ab2_ref
import gpu_harness as H
import tendency_windows as tw
from gpu_harness import (F32, F64, MASK_VALUE, SENTINEL, _assert_inputs_unchanged, _assert_pair, _assert_parent, _count_planes, _dev,  # noqa: F401
                         _filled, _free_hbm, _host_metrics, _id, _velocity_model as _model)
from momentum_ref import METRICS, cells_read, same_bits, tendencies
from special_values import pool

pytestmark = pytest.mark.gpu

KERNEL = tw.KERNELS["momentum"]
#         size            halo       element type
SMALL = [((10, 10, 1), (4, 4, 4), F64),            # one level: both vertical faces read a halo plane
         ((20, 12, 3), (1, 1, 1), F64),            # every stencil arm and both corners end on the last halo cell
         ((20, 12, 3), (1, 1, 1), F32),
         ((20, 12, 3), (3, 2, 1), F64),            # odd Hx: the element-aligned chunks
         ((20, 10, 9), (4, 4, 4), F64),            # more levels than twice the look-ahead and no multiple of it
         ((24, 11, 5), (4, 4, 4), F32),            # Ny odd: a partial last row tile (2 rows per item in Float32); 5 levels: look-ahead 2; rows on the 16-B grid
         ((48, 40, 6), (5, 5, 5), F64),            # the model halo
         ((48, 40, 6), (5, 5, 5), F32),
         ((50, 40, 3), (4, 4, 4), F32)]            # Nx = 2 mod 4: 8-B chunks
BIG = ((2304, 1283, 2), (4, 4, 4), F64)            # 1283 row tiles x 1152 chunks, more items than are resident; 1283 is odd
OFFSET = [SMALL[3], SMALL[4], SMALL[8]]            # every pointer one element off the 16-B grid: the GEN form by the pointers, not the rows
FIELDS = ("u", "v", "w")
SHARED = (*FIELDS, *METRICS, "dz_f")


def _ref(h, size, halo, n_fc=None, n_cf=None):
    """the reference parents (Gu, Gv) from sentinel-filled ones; with the count planes: masked to MASK_VALUE"""
    return H._ref(KERNEL, h, size, halo, () if n_fc is None else (n_fc, n_cf))


def _case(case):
    return H._case(KERNEL, case)


def _device(h, gpu, offset=0):
    return H._device(KERNEL, h, gpu, offset)


def _raw_call(osg, gpu, d, Gu, Gv, size, halo, n_fc=None, n_cf=None, value=0.0, scheme=0):
    return H._launch(osg, gpu, KERNEL, d, {"Gu": Gu, "Gv": Gv}, size, halo, counts=(n_fc, n_cf), value=value, scheme=scheme)


def _call(osg, gpu, d, size, halo, n_fc=None, n_cf=None, value=0.0, offset=0):
    """tpg_momentum_advection_tendency on the device arrays d into fresh sentinel-filled outputs -> the whole parents (Gu, Gv) on the host"""
    return H._call(osg, gpu, KERNEL, d, size, halo, None, (n_fc, n_cf), value, offset)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(c, 1) for c in OFFSET],
                         ids=[_id(c) for c in SMALL] + [_id(c) + "-offset" for c in OFFSET])
def test_interior_is_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, offset):
    """random data in every cell, the parents of Gu, Gv pre-filled with a sentinel: the whole parents equal the reference's -- the interior
    the rule, every halo cell still the sentinel -- and every input comes back as it was"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    for want in h["want"]:                                         # the reference parents themselves: sentinel exactly on the halo cells
        edge = np.ones(want.shape, bool)
        edge[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
        assert (want[edge] == SENTINEL).all() and not (want[~edge] == SENTINEL).any() and np.isfinite(want).all()
    assert same_bits(h["want"][0], h["want"][1]) > 0.9 * Nx * Ny * Nz
    d = _device(h, gpu, offset)
    _assert_pair(_call(osg, gpu, d, size, halo, offset=offset), h["want"], "parent")
    _assert_inputs_unchanged(d, h, "parent")


def test_more_items_than_are_resident(osg, gpu):
    """2304 x 1283 x 2: 1152 chunks x 1283 row tiles (642 with 2 rows per item, the last one partial), several rounds of resident blocks"""
    size, halo, dtype = BIG
    h = _case(BIG)
    d = _device(h, gpu)
    _assert_pair(_call(osg, gpu, d, size, halo), h["want"], "big")
    for k in FIELDS:
        _assert_parent(d[k].cpu().numpy(), h[k], ("big: unchanged", k))


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[0], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[0]) + "-offset"])
def test_no_cell_outside_the_stencil_is_read(osg, gpu, case, offset):
    """every cell of u, v, w and the eight metric planes that the rule does not read is NaN: the result has no NaN and equals the clean one"""
    size, halo, dtype = case
    h = _case(case)
    read = cells_read(size, halo)
    poisoned = {k: np.where(read[k], h[k], dtype(np.nan)) for k in read}
    assert set(read) == set(SHARED) - {"dz_f"}
    assert all(np.isnan(poisoned[k]).sum() == (~read[k]).sum() > 0 for k in poisoned)
    poisoned["dz_f"] = h["dz_f"]
    got = _call(osg, gpu, _device(poisoned, gpu, offset), size, halo, offset=offset)
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    _assert_pair(got, h["want"], "poisoned")


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[0], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[0]) + "-offset"])
def test_fused_mask_equals_the_reference_and_the_mask_pass(osg, gpu, case, offset):
    """with the count planes: (1) the reference with the mask; (2) the unmasked call followed by tpg_mask_immersed_fields on Gu (by n_fc) and
    Gv (by n_cf), zloc Center, bit for bit on the whole parents; without them nothing is masked (the first test)"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    nfc, ncf = _count_planes(case)
    want = _ref(h, size, halo, nfc, ncf)
    inner = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]        # noqa: E731
    assert (inner(want[0])[:, Ny - 1, Nx - 1] == dtype(MASK_VALUE)).all() and (inner(want[1])[:, Ny - 2, Nx - 1] == dtype(MASK_VALUE)).all()
    assert same_bits(inner(want[0])[:, 0, 0], inner(h["want"][0])[:, 0, 0]) == 0         # n < 0: nothing
    assert same_bits(inner(want[1])[:, 1, 0], inner(h["want"][1])[:, 1, 0]) == 0
    assert same_bits(want[0], h["want"][0]) > 0 and same_bits(want[1], h["want"][1]) > 0
    d = _device(h, gpu, offset)
    nd = [_dev(nfc, gpu, offset), _dev(ncf, gpu, offset)]
    _assert_pair(_call(osg, gpu, d, size, halo, n_fc=nd[0], n_cf=nd[1], value=MASK_VALUE, offset=offset), want, "fused mask")
    # the two-pass form, on what the unmasked call leaves (held equal to h["want"] by the first test)
    lib = osg._lib.lib()
    t = [_dev(h["want"][q], gpu, offset) for q in (0, 1)]
    osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table(t), 2, osg._lib.ptr_table(nd), (C.c_int8 * 2)(osg._lib.TPG_CENTER, osg._lib.TPG_CENTER),
                                                (C.c_double * 2)(MASK_VALUE, MASK_VALUE), Nx, Ny, Nz, *halo, osg._lib.ft_of(t[0].dtype),
                                                osg._lib.current_stream_ptr(gpu)))
    _assert_pair([x.cpu().numpy() for x in t], want, "two passes")


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[0], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[0]) + "-offset"])
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max planted in 1 % of the cells of u, v and w and 0.5 % of each metric plane (zero metrics among them:
    x / 0): bit for bit numpy's, which computes the same IEEE operations.  The stencil has about 35 field and 25 metric cells per node, so
    these shares leave the reference's interior more than 30 % finite with both NaN and Inf in it -- asserted before comparing"""
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

    planted = {"dz_f": h["dz_f"]}
    for name in FIELDS:
        planted[name] = plant(h[name], 0.01)
    for name in METRICS:
        planted[name] = plant(h[name], 0.005)
    # whatever the draw gave the small shapes: zero metrics of either sign, a NaN, an Inf and a -0 velocity cell in the interior
    planted["dx_fc"][Hy, Hx], planted["az_ff"][Hy + Ny - 1, Hx + Nx - 1], planted["az_cf"][Hy + 2, Hx + 2] = 0.0, -0.0, 0.0
    planted["u"][Hz, Hy + 1, Hx + 1], planted["v"][Hz, Hy + 3, Hx + 3], planted["u"][Hz, Hy + 5, Hx + 5] = np.nan, np.inf, -0.0
    want = _ref(planted, size, halo)
    for G in want:
        inner = G[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(inner).any() and np.isinf(inner).any() and np.isfinite(inner).mean() > 0.3
    _assert_pair(_call(osg, gpu, _device(planted, gpu, offset), size, halo, offset=offset), want, "special values")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_signs_of_zero(osg, gpu, dtype):
    """u = v = 0 everywhere, of either sign: every term is +-0 and the rule's leading minus signs are sign flips of the zeros the sums
    leave -- the bits numpy gives"""
    case = ((20, 12, 3), (1, 1, 1), dtype)
    size, halo, _ = case
    for sign in (1.0, -1.0):
        h = dict(_case(case))
        h["u"], h["v"] = np.zeros_like(h["u"]) * dtype(sign), np.zeros_like(h["v"]) * dtype(-sign)
        want = _ref(h, size, halo)
        assert all((G[1:-1, 1:-1, 1:-1] == 0).all() for G in want) and any(np.signbit(G[1:-1, 1:-1, 1:-1]).any() for G in want)
        _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), want, ("zeros", sign))


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched, the outputs keep the sentinel"""
    case = SMALL[1]
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.momentum_lib()
    err = lambda: lib.tpg_momentum_last_error().decode()          # noqa: E731
    out = [_dev(np.full(h["u"].shape, SENTINEL, dtype), gpu) for _ in range(2)]
    n = _dev(_count_planes(case)[0], gpu)
    assert _raw_call(osg, gpu, d, out[0], d["u"], size, halo) == -1 and err().startswith("Gv overlaps u")
    assert _raw_call(osg, gpu, d, d["w"], out[1], size, halo) == -1 and err().startswith("Gu overlaps w")
    assert _raw_call(osg, gpu, d, out[0], out[0], size, halo) == -1 and err() == "Gv overlaps Gu"
    assert _raw_call(osg, gpu, d, *out, size, halo, scheme=2) == -5 and "scheme 2 is not built" in err()
    assert _raw_call(osg, gpu, d, *out, size, halo, n_fc=n) == -1 and "together or not at all" in err()
    # Hz = 0: the same arrays read as a geometry without a vertical halo (3 + 2 levels x 14 x 22 cells fit the allocation)
    assert _raw_call(osg, gpu, d, *out, (20, 12, 5), (1, 1, 0)) == -5 and "Hz >= 1 needed (halo (1,1,0))" in err()
    with pytest.raises(osg._lib.TripolarHipError, match="TPG_ERR_UNSUPPORTED.*Hz >= 1 needed"):
        osg._lib.check_momentum(_raw_call(osg, gpu, d, *out, (20, 12, 5), (1, 1, 0)))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)
    _assert_inputs_unchanged(d, h, "refusals")


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
DT, CHI = 0.01, 0.1


@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)],
                         ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_two_steps_eagerly_and_as_a_graph_equal_the_references_composed(osg, gpu, size, halo, tdt, immersed):
    """filled u, v and w from compute_w_from_continuity, then twice: momentum tendency -> ab2_velocity_step_plan(fill_halos=True).  Eagerly,
    Gu, Gv, u, v and the previous tendencies after each step are the composition of momentum_ref, ab2_ref and the fill's; one captured graph
    of the two plans replayed twice from the start gives the same arrays.  On the immersed grid the mask in the call is
    mask_immersed_field's"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v, w, Gu, Gv, Gum, Gvm = _model(osg, gpu, size, halo, tdt, immersed)
    m, dz, (nfc, ncf) = _host_metrics(osg, KERNEL, grid, tdt)
    assert (nfc is not None) == immersed
    hw = w.data.cpu().numpy()
    tend = osg.momentum_advection_plan(u, v, w, Gu, Gv)
    step = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gum, Gvm, DT, chi=CHI, fill_halos=True)
    everything = [u, v, Gu, Gv, Gum, Gvm]
    start = [f.data.clone() for f in everything]
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]          # noqa: E731
    host = [f.data.cpu().numpy() for f in everything]
    for it in range(2):
        assert tend() is tend and step() is step
        u0, v0, Gu0, Gv0, Gum0, Gvm0 = host
        with np.errstate(all="ignore"):
            want_Gu, want_Gv = tendencies(u0, v0, hw, Gu0, Gv0, m, dz, size, halo, nfc, ncf, 0.0)
        new_u, prev_u, _ = ab2_ref.ab2_step(u0, want_Gu, Gum0, DT, CHI, ab2_ref.STORE, size, halo)
        new_v, prev_v, _ = ab2_ref.ab2_step(v0, want_Gv, Gvm0, DT, CHI, ab2_ref.STORE, size, halo)
        new_u, new_v = _filled(osg, u, cut(new_u), u0, u.boundary_conditions), _filled(osg, v, cut(new_v), v0, v.boundary_conditions)
        want = [new_u, new_v, want_Gu, want_Gv, prev_u, prev_v]
        for name, f, x in zip(("u", "v", "Gu", "Gv", "Gum", "Gvm"), everything, want):
            _assert_parent(f.data.cpu().numpy(), x, (name, it))
        assert same_bits(cut(new_u), cut(u0)) > 0 and same_bits(cut(want_Gv), cut(Gv0)) > 0          # the step and the tendency changed something
        host = want
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
    _assert_parent(w.data.cpu().numpy(), hw, "w unchanged")
    if immersed:                                                   # the mask value of the call is the mask pass's
        raw = osg.momentum_advection_tendency(u, v, w, mask_immersed=False)
        masked = osg.momentum_advection_tendency(u, v, w)
        assert all(same_bits(a.data.cpu().numpy(), b.data.cpu().numpy()) > 0 for a, b in zip(raw, masked))
        osg.mask_immersed_field(list(raw), 0)
        for a, b in zip(raw, masked):
            _assert_parent(a.data.cpu().numpy(), b.data.cpu().numpy(), "mask pass")


def test_out_is_allocated_or_given_and_filled(osg, gpu):
    """`out=None` allocates an XFaceField and a YFaceField whose halos stay zero; a given pair is written and, with fill_halos, filled"""
    size, halo, tdt = (20, 12, 3), (3, 2, 1), torch.float64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v, w, Gu, Gv, _, _ = _model(osg, gpu, size, halo, tdt, False)
    m, dz, _ = _host_metrics(osg, KERNEL, grid, tdt)
    hu, hv, hw = (f.data.cpu().numpy() for f in (u, v, w))
    zero = np.zeros_like(hu)
    want = tendencies(hu, hv, hw, zero, zero, m, dz, size, halo)
    out = osg.momentum_advection_tendency(u, v, w)
    assert len(out) == 2 and out[0].loc == (osg.Face, osg.Center, osg.Center) and out[1].loc == (osg.Center, osg.Face, osg.Center)
    assert all(o.grid is grid for o in out)
    _assert_pair([o.data.cpu().numpy() for o in out], want, "allocated")
    given = osg.momentum_advection_tendency(u, v, w, out=(Gu, Gv), fill_halos=True)
    assert given[0] is Gu and given[1] is Gv
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    for f, x in zip((Gu, Gv), want):
        assert same_bits(f.interior().cpu().numpy().reshape(x[cut].shape)[:, :Ny - 1], x[cut][:, :Ny - 1]) == 0     # the fold may rewrite row Ny
        assert bool((f.data[Hz:Hz + Nz, Hy:Hy + Ny, :Hx] != 0).any())                                              # the halos were filled
