"""GPU tests of the momentum advection tendency with the WENO5-upwinded vorticity term: tpg_weno_momentum_advection_tendency through the C
ABI, and weno_momentum_advection_tendency / weno_momentum_advection_plan through the package.  Compared BIT FOR BIT with
tests/weno_momentum_ref.py (numpy in the fields' type: every operation of the rule is one correctly rounded IEEE operation, so the reference
is exact and there is no tolerance anywhere in this file); NaNs compare by NaN-ness; whole parents are compared: the halo cells of Gu, Gv
against a sentinel, and the inputs must come back unchanged.  Inputs are random in every cell, dz_f and the metrics in [0.5, 2], so a wrong
face index or metric cell cannot hide.

Shapes, the smallest at which each path can go wrong, and what each can catch:
- 10 x 10 x 1, halo 4: one level -- both vertical faces read a halo plane, the level loop runs once.
- 20 x 12 x 3, halo (3, 3, 1), Float64 and Float32: the minimum halo -- every arm of the two crosses and the corners end on the last halo
  cell (an index one too far leaves the row or reads a poisoned cell), and Hx is odd: the element-aligned chunks (Float32: 4 wide).
- 20 x 10 x 9, halo 4: more levels than twice any look-ahead of the compile-time variants and no multiple of it.
- 24 x 11 x 5, halo 4, Float32 AND Float64: Ny odd, a partial last row tile.  The committed kernel takes 2 rows per item in both types
  (the momentum kernel takes 1 in Float64, so its list has this shape in Float32 only): the rows of the tile past the interior are
  computed on clamped offsets and must store nothing.
- 48 x 40 x 6, halo 5, both types: the model halo.
- 50 x 40 x 3, halo 4, Float32: Nx = 2 mod 4, 8-B chunks -- W = 2, where the third Z east of a chunk comes from the SECOND lane east.
- three of them with every pointer one element off the 16-B grid: the element-aligned form by the pointers, not the rows.
- 140 x 6 x 2 (Float64) and 280 x 6 x 2 (Float32), halo 4: 70 chunks in a row.  The kernel numbers its items (row tile, chunk) with the
  chunk fastest, 64 to a wave, and a lane takes the Z beside its chunk from the lanes west and east of it unless that lane is in another
  wave or holds a chunk of another row tile.  70 is more than one wave and no multiple of 64: the wave edges fall inside a row at a
  different chunk in each of the 3 row tiles (64 | 58 | 52), and each row's end -- the periodic seam, whose Z lie in the halo columns --
  falls inside a wave (lanes 5 | 6, 11 | 12), where the neighbouring lane is there but holds the wrong chunk.
- 1024 x 515 x 2: 512 chunks x 258 row tiles = 132 096 items, more than are resident (the kernel runs one wave per SIMD: 256 CUs x 4 x 64 =
  65 536 items a round), the last tile partial.  The momentum kernel's 2304 x 1283 x 2 is five times the reference arithmetic for the same
  property."""
import ctypes as C

import numpy as np
import pytest
import torch

import ab2_ref
import gpu_harness as H
import tendency_windows as tw
from gpu_harness import (F32, F64, MASK_VALUE, SENTINEL, _assert_inputs_unchanged, _assert_pair, _assert_parent, _count_planes, _dev,  # noqa: F401
                         _filled, _free_hbm, _host_metrics, _id, _velocity_model as _model)
from special_values import pool
from weno_momentum_ref import METRICS, cells_read, dependence_window, same_bits, tendencies, terms, zeta_at
from weno_ref import face_value

pytestmark = pytest.mark.gpu

KERNEL = tw.KERNELS["weno_momentum"]
#         size            halo       element type
SMALL = [((10, 10, 1), (4, 4, 4), F64),
         ((20, 12, 3), (3, 3, 1), F64),
         ((20, 12, 3), (3, 3, 1), F32),
         ((20, 10, 9), (4, 4, 4), F64),
         ((24, 11, 5), (4, 4, 4), F32),
         ((24, 11, 5), (4, 4, 4), F64),
         ((48, 40, 6), (5, 5, 5), F64),
         ((48, 40, 6), (5, 5, 5), F32),
         ((50, 40, 3), (4, 4, 4), F32),
         ((140, 6, 2), (4, 4, 4), F64),            # 70 chunks a row: wave edges inside a row, row ends inside a wave
         ((280, 6, 2), (4, 4, 4), F32)]
BIG = ((1024, 515, 2), (4, 4, 4), F64)
OFFSET = [SMALL[1], SMALL[3], SMALL[8]]            # every pointer one element off the 16-B grid
FIELDS = ("u", "v", "w")
SHARED = (*FIELDS, *METRICS, "dz_f")


def _ref(h, size, halo, n_fc=None, n_cf=None):
    """the reference parents (Gu, Gv) from sentinel-filled ones; with the count planes: masked to MASK_VALUE"""
    return H._ref(KERNEL, h, size, halo, () if n_fc is None else (n_fc, n_cf))


def _case(case):
    return H._case(KERNEL, case)


def _device(h, gpu, offset=0):
    return H._device(KERNEL, h, gpu, offset)


def _raw_call(osg, gpu, d, Gu, Gv, size, halo, n_fc=None, n_cf=None, value=0.0, shift_u=0):
    return H._launch(osg, gpu, KERNEL, d, {"Gu": Gu, "Gv": Gv}, size, halo, counts=(n_fc, n_cf), value=value, shift=("u", shift_u))


def _call(osg, gpu, d, size, halo, n_fc=None, n_cf=None, value=0.0, offset=0):
    """tpg_weno_momentum_advection_tendency on the device arrays d into fresh sentinel-filled outputs -> the whole parents (Gu, Gv) on the host"""
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
    """1024 x 515 x 2: 512 chunks x 258 row tiles (the last one partial), more than two rounds of resident blocks"""
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


@pytest.mark.parametrize("v_positive", [True, False], ids=["vhat>=0", "vhat<0"])
@pytest.mark.parametrize("u_positive", [True, False], ids=["uhat>=0", "uhat<0"])
def test_domain_of_dependence_without_an_oracle(osg, gpu, v_positive, u_positive):
    """u and v of one sign each (so vhat and uhat have one sign everywhere); one cell of u or v scaled by 1.25: the nodes of Gu and Gv whose
    bits move are EXACTLY dependence_window's -- the upwind window, no node more and none less -- for a cell in the middle, a cell of the
    west and one of the east halo (read across the periodic seam) and a cell of the Zipper rows north of the interior.  No reference value is compared"""
    size, halo, dtype = (20, 12, 3), (3, 3, 1), F64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = dict(_case((size, halo, dtype)))
    rng = np.random.default_rng([5, v_positive, u_positive])
    h["u"] = (rng.uniform(0.5, 1, h["u"].shape) * (1 if u_positive else -1)).astype(dtype)
    h["v"] = (rng.uniform(0.5, 1, h["v"].shape) * (1 if v_positive else -1)).astype(dtype)
    t = terms(h["u"], h["v"], h["w"], {k: h[k] for k in METRICS}, h["dz_f"], size, halo)
    assert ((t["vhat"] >= 0) == v_positive).all() and ((t["uhat"] >= 0) == u_positive).all()
    base = _call(osg, gpu, _device(h, gpu), size, halo)
    # middle; west halo, column -1; east halo, column Nx + 2 (both read across the periodic seam); Zipper row Ny + 2
    cells = [(Hz + 1, Hy + 5, Hx + 9), (Hz + 1, Hy + 6, Hx - 2), (Hz + 1, Hy + 3, Hx + Nx + 1), (Hz, Hy + Ny + 1, Hx + 4)]
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    seen = set()
    for name in ("u", "v"):
        for cell in cells:
            b = dict(h)
            b[name] = h[name].copy()
            b[name][cell] *= dtype(1.25)
            changed = np.zeros(h[name].shape, bool)
            changed[cell] = True
            window = dependence_window(name, changed, size, halo, v_positive, u_positive)
            got = _call(osg, gpu, _device(b, gpu), size, halo)
            for q, G in enumerate(("Gu", "Gv")):
                moved = got[q][cut].view(np.uint64) != base[q][cut].view(np.uint64)
                assert np.array_equal(moved, window[q]), (name, cell, G, np.argwhere(moved != window[q])[:8])
                seen.add((name, cell, G, int(window[q].sum())))
    # some windows are empty (a cell of row Ny + 2 is beyond every Gv node's reach, column -1 beyond a right-biased window's): most are not
    assert len(seen) == 16 and sum(n > 0 for *_, n in seen) >= 8, sorted(seen)


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


def _planted(case):
    """the case with +-0, subnormals, +-Inf, NaN, +-max planted in 1 % of the cells of u, v and w and 0.5 % of each metric plane"""
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
    if dtype == F32:                                               # Float32 subnormals, whatever the draw gave
        planted["u"][Hz, Hy + 4, Hx + 7], planted["v"][Hz, Hy + 6, Hx + 2] = np.float32(1e-41), np.float32(-3e-45)
    return planted


@pytest.mark.parametrize("case,offset", [(c, 0) for c in SMALL] + [(OFFSET[0], 1)], ids=[_id(c) for c in SMALL] + [_id(OFFSET[0]) + "-offset"])
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals (Float32's too), +-Inf, NaN, +-max planted in read cells, zero metrics among them (x / 0, and az_ff = 0: a
    non-finite Z, which reaches every node whose window holds it): bit for bit numpy's, which computes the same IEEE operations.  The
    stencil has about 60 field and 45 metric cells per node, so these shares leave the reference's interior more than 30 % finite with
    both NaN and Inf or NaN alone in it -- asserted before comparing"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    planted = _planted(case)
    want = _ref(planted, size, halo)
    for G in want:
        inner = G[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(inner).any() and np.isfinite(inner).mean() > 0.3
    _assert_pair(_call(osg, gpu, _device(planted, gpu, offset), size, halo, offset=offset), want, "special values")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_selection_at_minus_zero_and_nan(osg, gpu, dtype):
    """`>= 0` is true for -0 and false for NaN.  v = -0 everywhere makes vhat = -0 at every node: the LEFT-biased window Z[j-2..j+2] is
    taken, hu is +-0 with the sign of that window's zr -- and with az_ff = 0 planted (a non-finite Z) a right-biased choice would give NaN at
    other nodes than the left-biased one does.  The same with u = -0 for uhat.  With NaN planted in v (u) the transverse velocity is NaN at
    the nodes around it: the rule takes the right-biased window there, and NaN * zr is NaN either way, so only NaN-ness is observable at
    those nodes -- it is compared.  All bit for bit numpy's"""
    case = ((20, 12, 3), (3, 3, 1), dtype)
    size, halo, _ = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    base = _case(case)
    m = {k: base[k].copy() for k in METRICS}
    m["az_ff"][Hy + 4, Hx + 6], m["az_ff"][Hy + 8, Hx + 13] = 0.0, 0.0
    for zeroed, other, axis in (("v", "u", 0), ("u", "v", 1)):
        h = dict(base, **m)
        h[zeroed] = np.zeros_like(base[zeroed]) * dtype(-1.0)
        t = terms(h["u"], h["v"], h["w"], m, h["dz_f"], size, halo)
        vel = t["vhat"] if zeroed == "v" else t["uhat"]
        assert (vel == 0).all() and np.signbit(vel).all()
        # what the other choice would have given: the right-biased window
        with np.errstate(all="ignore"):
            z = [zeta_at(h["u"], h["v"], m, size, halo, *((0, d) if axis == 0 else (d, 0))) for d in range(-2, 4)]
            right = face_value(z[5], z[4], z[3], z[2], z[1])
        left = t["zru"] if zeroed == "v" else t["zrv"]
        assert (np.isnan(left) != np.isnan(right)).any() and (np.signbit(left) != np.signbit(right)).any()
        want = _ref(h, size, halo)
        _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), want, ("minus zero", zeroed))
    for name in ("v", "u"):
        h = dict(base)
        h[name] = base[name].copy()
        h[name][Hz + 1, Hy + 5, Hx + 8] = np.nan
        want = _ref(h, size, halo)
        assert all(0 < np.isnan(G).sum() < 200 for G in want)
        _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), want, ("nan", name))


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched, the outputs keep the sentinel"""
    case = SMALL[1]
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.weno_momentum_lib()
    err = lambda: lib.tpg_weno_momentum_last_error().decode()     # noqa: E731
    out = [_dev(np.full(h["u"].shape, SENTINEL, dtype), gpu) for _ in range(2)]
    n = _dev(_count_planes(case)[0], gpu)
    assert _raw_call(osg, gpu, d, out[0], d["u"], size, halo) == -1 and err().startswith("Gv overlaps u")
    assert _raw_call(osg, gpu, d, d["w"], out[1], size, halo) == -1 and err().startswith("Gu overlaps w")
    assert _raw_call(osg, gpu, d, out[0], out[0], size, halo) == -1 and err() == "Gv overlaps Gu"
    assert _raw_call(osg, gpu, d, *out, size, halo, n_fc=n) == -1 and "together or not at all" in err()
    assert _raw_call(osg, gpu, d, *out, size, halo, shift_u=4) == -1 and err() == "u, v or w pointer not aligned to its element type"   # half an element off
    # thin halos: the same arrays read as geometries of the same row pitch and plane with a smaller halo (they fit the allocation)
    assert _raw_call(osg, gpu, d, *out, (22, 12, 3), (2, 3, 1)) == -5 and "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,3,1))" in err()
    assert _raw_call(osg, gpu, d, *out, (20, 14, 3), (3, 2, 1)) == -5 and "needed (halo (3,2,1))" in err()
    assert _raw_call(osg, gpu, d, *out, (20, 12, 5), (3, 3, 0)) == -5 and "needed (halo (3,3,0))" in err()
    with pytest.raises(osg._lib.TripolarHipError, match="TPG_ERR_UNSUPPORTED.*Hz >= 1 needed"):
        osg._lib.check_weno_momentum(_raw_call(osg, gpu, d, *out, (20, 12, 5), (3, 3, 0)))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)
    _assert_inputs_unchanged(d, h, "refusals")


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
DT, CHI = 0.01, 0.1


@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)],
                         ids=["48x40x6-h5-f64", "50x40x3-h4-f32"])
def test_two_steps_eagerly_and_as_a_graph_equal_the_references_composed(osg, gpu, size, halo, tdt, immersed):
    """filled u, v and w from compute_w_from_continuity, then twice: this tendency -> ab2_velocity_step_plan(fill_halos=True).  Eagerly, Gu,
    Gv, u, v and the previous tendencies after each step are the composition of weno_momentum_ref, ab2_ref and the fill's; one captured
    graph of the two plans replayed twice from the start gives the same arrays.  On the immersed grid the mask in the call is
    mask_immersed_field's"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v, w, Gu, Gv, Gum, Gvm = _model(osg, gpu, size, halo, tdt, immersed)
    m, dz, (nfc, ncf) = _host_metrics(osg, KERNEL, grid, tdt)
    assert (nfc is not None) == immersed
    hw = w.data.cpu().numpy()
    tend = osg.weno_momentum_advection_plan(u, v, w, Gu, Gv)
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
        raw = osg.weno_momentum_advection_tendency(u, v, w, mask_immersed=False)
        masked = osg.weno_momentum_advection_tendency(u, v, w)
        assert all(same_bits(a.data.cpu().numpy(), b.data.cpu().numpy()) > 0 for a, b in zip(raw, masked))
        osg.mask_immersed_field(list(raw), 0)
        for a, b in zip(raw, masked):
            _assert_parent(a.data.cpu().numpy(), b.data.cpu().numpy(), "mask pass")


def test_out_is_allocated_or_given_and_filled(osg, gpu):
    """`out=None` allocates an XFaceField and a YFaceField whose halos stay zero; a given pair is written and, with fill_halos, filled"""
    size, halo, tdt = (20, 12, 3), (3, 3, 1), torch.float64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v, w, Gu, Gv, _, _ = _model(osg, gpu, size, halo, tdt, False)
    m, dz, _ = _host_metrics(osg, KERNEL, grid, tdt)
    hu, hv, hw = (f.data.cpu().numpy() for f in (u, v, w))
    zero = np.zeros_like(hu)
    with np.errstate(all="ignore"):
        want = tendencies(hu, hv, hw, zero, zero, m, dz, size, halo)
    out = osg.weno_momentum_advection_tendency(u, v, w)
    assert len(out) == 2 and out[0].loc == (osg.Face, osg.Center, osg.Center) and out[1].loc == (osg.Center, osg.Face, osg.Center)
    assert all(o.grid is grid for o in out)
    _assert_pair([o.data.cpu().numpy() for o in out], want, "allocated")
    given = osg.weno_momentum_advection_tendency(u, v, w, out=(Gu, Gv), fill_halos=True)
    assert given[0] is Gu and given[1] is Gv
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    for f, x in zip((Gu, Gv), want):
        assert same_bits(f.interior().cpu().numpy().reshape(x[cut].shape)[:, :Ny - 1], x[cut][:, :Ny - 1]) == 0     # the fold may rewrite row Ny
        assert bool((f.data[Hz:Hz + Nz, Hy:Hy + Ny, :Hx] != 0).any())                                              # the halos were filled
