"""GPU tests of the momentum advection tendency with upwinding in every term: tpg_weno_vi_momentum_advection_tendency through the C ABI,
and weno_vi_momentum_advection_tendency / weno_vi_momentum_advection_plan through the package.  Compared BIT FOR BIT with
tests/weno_vi_ref.py (numpy in the fields' type: every operation of the rule is one correctly rounded IEEE operation, so the reference is
exact and there is no tolerance anywhere in this file); NaNs compare by NaN-ness; whole parents are compared: the halo cells of Gu, Gv
against a sentinel, and the inputs must come back unchanged.  Inputs are random in every cell, dz_c and the metrics in [0.5, 2], so a wrong
face index or metric cell cannot hide.

Shapes, the smallest at which each path can go wrong:
- (4, 3, 1) at halo (3, 3, 1) and (4, 4, 5) at halo (4, 4, 4): the smallest served, every arm ends on the last halo cell.
- 12 x 5 x Nz for Nz = 1, 2, 3, 4, 5, 6, 7, 9 -- every class of the z-faces' order table on both sides of the column -- in the three chunk
  forms (halo 4 on the 16-B grid; the same with every pointer one element off it; halo (3, 3, 1): an odd Hx), Float32 and Float64.  Ny = 5
  is odd: the first launch takes two rows per item and its last tile is partial.  10 x 5 x 6 in Float32: 8-B chunks (Nx = 2 mod 4).
- 130 x 4 x 2 in Float64 and 260 x 4 x 2 in Float32: 65 chunks a row, so a wave edge (64 | 65), a row end and the periodic seam fall inside
  the arms of the first launch's shared Z and of the second launch's rows.
- every case compares the rows Ny, Ny - 1, Ny - 2, whose arms reach the rows Ny + 1 .. Ny + 3, random like every other cell.
Its latitude bands (40 x 24 x 7) and its test past 2^31 elements are tests/test_gpu_tendency_edges.py's, from its row of the adapter table."""
import ctypes as C

import numpy as np
import pytest
import torch

import ab2_ref
import gpu_harness as H
import tendency_windows as tw
from gpu_harness import (F32, F64, MASK_VALUE, SENTINEL, _assert_inputs_unchanged, _assert_pair, _assert_parent, _count_planes, _dev,  # noqa: F401
                         _filled, _free_hbm, _host_metrics, _velocity_model as _model)
from special_values import pool
from weno_vi_ref import METRICS, cells_read, dependence_window, same_bits, tendencies, terms

pytestmark = pytest.mark.gpu

KERNEL = tw.KERNELS["weno_vi"]
NZS = (1, 2, 3, 4, 5, 6, 7, 9)
FORMS = {"aligned": ((4, 4, 4), 0), "offset": ((4, 4, 4), 1), "oddHx": ((3, 3, 1), 0)}
LEVELS = [(((12, 5, nz), halo, dtype), off, f"12x5x{nz}-{form}-{'f64' if dtype == F64 else 'f32'}")
          for nz in NZS for form, (halo, off) in FORMS.items() for dtype in (F64, F32)]
EDGES = [(((4, 3, 1), (3, 3, 1), F64), 0, "4x3x1-h331-f64"), (((4, 3, 1), (3, 3, 1), F32), 0, "4x3x1-h331-f32"),
         (((4, 4, 5), (4, 4, 4), F64), 0, "4x4x5-h444-f64"), (((4, 4, 5), (4, 4, 4), F32), 0, "4x4x5-h444-f32"),
         (((10, 5, 6), (4, 4, 4), F32), 0, "10x5x6-h444-f32-8B"),
         (((130, 4, 2), (4, 4, 4), F64), 0, "130x4x2-h444-f64"), (((260, 4, 2), (4, 4, 4), F32), 0, "260x4x2-h444-f32"),
         (((130, 4, 2), (3, 3, 1), F64), 0, "130x4x2-h331-f64")]
ALL = LEVELS + EDGES
SOME = [c for c in ALL if c[2] in ("12x5x9-aligned-f64", "12x5x9-oddHx-f32", "12x5x7-offset-f64", "12x5x4-aligned-f32", "12x5x1-oddHx-f64",
                                   "130x4x2-h444-f64", "260x4x2-h444-f32", "10x5x6-h444-f32-8B")]
FIELDS = ("u", "v", "w")
SHARED = (*FIELDS, *METRICS, "dz_c")


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
    """tpg_weno_vi_momentum_advection_tendency on the device arrays d into fresh sentinel-filled outputs -> the whole parents (Gu, Gv) on the host"""
    return H._call(osg, gpu, KERNEL, d, size, halo, None, (n_fc, n_cf), value, offset)


def _params(cases):
    return pytest.mark.parametrize("case,offset", [(c, o) for c, o, _ in cases], ids=[i for *_, i in cases])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
@_params(ALL)
def test_interior_is_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, offset):
    """random data in every cell, the parents of Gu, Gv pre-filled with a sentinel: the whole parents equal the reference's -- the interior
    the rule, every halo cell still the sentinel -- and every input comes back as it was"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    for want in h["want"]:
        edge = np.ones(want.shape, bool)
        edge[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
        assert (want[edge] == SENTINEL).all() and not (want[~edge] == SENTINEL).any() and np.isfinite(want).all()
    d = _device(h, gpu, offset)
    _assert_pair(_call(osg, gpu, d, size, halo, offset=offset), h["want"], "parent")
    _assert_inputs_unchanged(d, h, "parent")


@_params(SOME)
def test_no_cell_outside_the_stencil_is_read(osg, gpu, case, offset):
    """every cell of u, v, w and the eight metric planes that the rule does not read is NaN: the result has no NaN and equals the clean one"""
    size, halo, dtype = case
    h = _case(case)
    read = cells_read(size, halo)
    poisoned = {k: np.where(read[k], h[k], dtype(np.nan)) for k in read}
    assert set(read) == set(SHARED) - {"dz_c"}
    assert all(np.isnan(poisoned[k]).sum() == (~read[k]).sum() > 0 for k in poisoned)
    poisoned["dz_c"] = h["dz_c"]
    got = _call(osg, gpu, _device(poisoned, gpu, offset), size, halo, offset=offset)
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    _assert_pair(got, h["want"], "poisoned")


@pytest.mark.parametrize("positive", [True, False], ids=["positive", "negative"])
def test_domain_of_dependence_without_an_oracle(osg, gpu, positive):
    """u, v and w of one sign (so every advecting velocity has one sign everywhere); one cell of u or v scaled by 1.25: the nodes of Gu and
    Gv whose bits move are EXACTLY dependence_window's -- the upwind windows in x, y and z, no node more and none less -- for a cell in the
    middle, a cell of the west halo (read across the periodic seam), a cell of the Zipper rows and a cell of the bottom halo plane.  No
    reference value is compared"""
    size, halo, dtype = (12, 9, 9), (3, 3, 1), F64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = dict(_case((size, halo, dtype)))
    for k in FIELDS:
        h[k] = (1 if positive else -1) * (np.abs(h[k]) * 0.5 + 0.5)
    t = terms(h["u"], h["v"], h["w"], {k: h[k] for k in METRICS}, h["dz_c"], size, halo)
    assert ((t["Wu"] >= 0) == positive).all() and ((t["Wv"] >= 0) == positive).all()
    base = _call(osg, gpu, _device(h, gpu), size, halo)
    cells = [(Hz + 4, Hy + 4, Hx + 5), (Hz + 1, Hy + 3, Hx - 2), (Hz + 7, Hy + Ny + 1, Hx + 6), (0, Hy + 2, Hx + 3)]
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    sizes = []
    for name in ("u", "v"):
        for cell in cells:
            b = dict(h)
            b[name] = h[name].copy()
            b[name][cell] *= dtype(1.25)
            changed = np.zeros(h[name].shape, bool)
            changed[cell] = True
            window = dependence_window(name, changed, size, halo, positive, positive, positive)
            got = _call(osg, gpu, _device(b, gpu), size, halo)
            for q, G in enumerate(("Gu", "Gv")):
                moved = got[q][cut].view(np.uint64) != base[q][cut].view(np.uint64)
                assert np.array_equal(moved, window[q]), (name, cell, G, np.argwhere(moved != window[q])[:8])
                sizes.append(int(window[q].sum()))
    assert len(sizes) == 16 and sum(n > 0 for n in sizes) >= 10 and max(sizes) >= 15, sizes


@_params(SOME)
def test_fused_mask_equals_the_reference_and_the_mask_pass(osg, gpu, case, offset):
    """with the count planes: (1) the reference with the mask; (2) the unmasked result followed by tpg_mask_immersed_fields on Gu (by n_fc)
    and Gv (by n_cf), bit for bit on the whole parents; without them nothing is masked (the first test)"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    nfc, ncf = _count_planes(case, varied=False)
    want = _ref(h, size, halo, nfc, ncf)
    inner = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]        # noqa: E731
    assert (inner(want[0])[:, Ny - 1, Nx - 1] == dtype(MASK_VALUE)).all() and (inner(want[1])[:, Ny - 2, Nx - 1] == dtype(MASK_VALUE)).all()
    assert same_bits(inner(want[0])[:, 0, 0], inner(h["want"][0])[:, 0, 0]) == 0         # n < 0: nothing
    assert same_bits(want[0], h["want"][0]) > 0 and same_bits(want[1], h["want"][1]) > 0
    d = _device(h, gpu, offset)
    nd = [_dev(nfc, gpu, offset), _dev(ncf, gpu, offset)]
    _assert_pair(_call(osg, gpu, d, size, halo, n_fc=nd[0], n_cf=nd[1], value=MASK_VALUE, offset=offset), want, "fused mask")
    lib = osg._lib.lib()
    t = [_dev(h["want"][q], gpu, offset) for q in (0, 1)]
    osg._lib.check(lib.tpg_mask_immersed_fields(osg._lib.ptr_table(t), 2, osg._lib.ptr_table(nd), (C.c_int8 * 2)(osg._lib.TPG_CENTER, osg._lib.TPG_CENTER),
                                                (C.c_double * 2)(MASK_VALUE, MASK_VALUE), Nx, Ny, Nz, *halo, osg._lib.ft_of(t[0].dtype),
                                                osg._lib.current_stream_ptr(gpu)))
    _assert_pair([x.cpu().numpy() for x in t], want, "two passes")


def _planted(case):
    """the case with +-0, subnormals, +-Inf, NaN, +-max planted in 0.5 % of the cells of u, v and w and 0.3 % of each metric plane"""
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
    for name in FIELDS:
        planted[name] = plant(h[name], 0.005)
    for name in METRICS:
        planted[name] = plant(h[name], 0.003)
    # whatever the draw gave: zero metrics of either sign, a NaN, an Inf and a -0 velocity cell in the interior
    planted["dx_fc"][Hy, Hx], planted["az_fc"][Hy + Ny - 1, Hx + Nx - 1], planted["az_cf"][Hy + 2, Hx + 2] = 0.0, -0.0, 0.0
    planted["u"][Hz, Hy + 1, Hx + 1], planted["v"][Hz, Hy + 3, Hx + 3], planted["u"][Hz, Hy + 2, Hx + 3] = np.nan, np.inf, -0.0
    if dtype == F32:                                               # Float32 subnormals, whatever the draw gave
        planted["u"][Hz, Hy + 3, Hx + 7], planted["v"][Hz, Hy + 1, Hx + 2] = np.float32(1e-41), np.float32(-3e-45)
    return planted


BIGGER = [(((48, 40, 9), (5, 5, 5), F64), 0, "48x40x9-h5-f64"), (((48, 40, 9), (4, 4, 4), F32), 0, "48x40x9-h4-f32"),
          (((50, 40, 6), (3, 3, 1), F32), 1, "50x40x6-h331-f32-offset")]


@_params(BIGGER)
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals (Float32's too), +-Inf, NaN, +-max planted in read cells, zero metrics among them (x / 0): bit for bit numpy's,
    which computes the same IEEE operations.  The stencil has about a hundred cells per node, so these shares leave the reference's
    interior more than 20 % finite with NaN in it -- asserted before comparing.  48 x 40: the model halo 5, more than one block"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    planted = _planted(case)
    want = _ref(planted, size, halo)
    for G in want:
        inner = G[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(inner).any() and np.isfinite(inner).mean() > 0.2
    _assert_pair(_call(osg, gpu, _device(planted, gpu, offset), size, halo, offset=offset), want, "special values")
    h = _case(case)                                                # and the clean case of the same shape
    _assert_pair(_call(osg, gpu, _device(h, gpu, offset), size, halo, offset=offset), h["want"], "clean")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_selection_at_minus_zero_and_nan(osg, gpu, dtype):
    """`>= 0` is true for -0 and false for NaN, for uu, vv, Wu and Wv, at z-faces of every order (Nz = 9).
    - u = -0 in one cell of three: uu = -0 takes the LEFT-biased windows of dur and kur.  uu multiplies dur away, but kur shows: the
      reference's kur there is the left-biased value and differs from the right-biased one (asserted), and the kernel equals the
      reference.  The same for v.
    - w = +-0 in every cell: Wu, Wv are +-0 (both signs occur: C4 of (+0, -0, -0, +0) is -0), FZ = 0 * ZF is observable where ZF is not
      finite: u and v carry an Inf in every column, which only the windows of one side hold.  A choice by the sign bit would give other
      NaNs (asserted on the reference with w = -tiny).
    - NaN planted in u, v, w: the advecting velocity is NaN at the nodes around it, the right-biased window is taken; only NaN-ness is
      observable there, and it is compared.  All bit for bit numpy's"""
    case = ((12, 9, 9), (3, 3, 1), dtype)
    size, halo, _ = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    base = _case(case)
    m = {k: base[k] for k in METRICS}
    rng = np.random.default_rng(23)
    for zeroed in ("u", "v"):
        h = dict(base)
        h[zeroed] = np.where(rng.random(base[zeroed].shape) < 1 / 3, dtype(-0.0), base[zeroed])
        t = terms(h["u"], h["v"], h["w"], m, h["dz_c"], size, halo)
        vel = h[zeroed][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        at = (vel == 0) & np.signbit(vel)
        assert at.sum() > 100
        flipped = dict(h)
        flipped[zeroed] = np.where(h[zeroed] == 0, dtype(-1e-30), h[zeroed])          # what a choice by the sign would have taken
        t2 = terms(flipped["u"], flipped["v"], flipped["w"], m, h["dz_c"], size, halo)
        key = "kur" if zeroed == "u" else "kvr"
        assert same_bits(t[key][at], t2[key][at]) > 0.9 * at.sum()
        _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), _ref(h, size, halo), ("minus zero", zeroed))
    h = dict(base)
    h["w"] = np.where(rng.random(base["w"].shape) < 0.5, dtype(-0.0), dtype(0.0))
    for name in ("u", "v"):
        a = base[name].copy()
        a[Hz + 2, Hy:Hy + Ny, Hx:Hx + Nx] = np.inf                 # level 3: face 6 holds it in its left window only, face 2 in neither
        h[name] = a
    t = terms(h["u"], h["v"], h["w"], m, h["dz_c"], size, halo)
    assert np.signbit(t["Wu"]).any() and not np.signbit(t["Wu"]).all() and (t["Wu"] == 0).all()
    neg = dict(h, w=np.full_like(h["w"], -1e-30))
    t2 = terms(neg["u"], neg["v"], neg["w"], m, h["dz_c"], size, halo)
    assert (np.isnan(t["FZu"]) != np.isnan(t2["FZu"])).any() and (np.isnan(t["FZv"]) != np.isnan(t2["FZv"])).any()
    _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), _ref(h, size, halo), "zero w")
    for name in FIELDS:
        h = dict(base)
        h[name] = base[name].copy()
        for level in (Hz, Hz + 1, Hz + 2, Hz + 4, Hz + 8):         # beside faces of order 2 (the wall), 1, 3, 5 and the top wall
            h[name][level, Hy + 4, Hx + (level % 5) + 3] = np.nan
        want = _ref(h, size, halo)
        assert all(0 < np.isnan(G).sum() < 400 for G in want)
        _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), want, ("nan", name))


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched -- neither launch --, the outputs keep the sentinel"""
    case = ((12, 5, 3), (3, 3, 1), F64)
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.weno_vi_lib()
    err = lambda: lib.tpg_weno_vi_last_error().decode()           # noqa: E731
    out = [_dev(np.full(h["u"].shape, SENTINEL, dtype), gpu) for _ in range(2)]
    n = _dev(_count_planes(case, varied=False)[0], gpu)
    assert _raw_call(osg, gpu, d, out[0], d["u"], size, halo) == -1 and err().startswith("Gv overlaps u")
    assert _raw_call(osg, gpu, d, d["w"], out[1], size, halo) == -1 and err().startswith("Gu overlaps w")
    assert _raw_call(osg, gpu, d, out[0], out[0], size, halo) == -1 and err() == "Gv overlaps Gu"
    assert _raw_call(osg, gpu, d, *out, size, halo, n_fc=n) == -1 and "together or not at all" in err()
    assert _raw_call(osg, gpu, d, *out, size, halo, shift_u=4) == -1 and err() == "u, v or w pointer not aligned to its element type"
    assert _raw_call(osg, gpu, d, *out, (14, 5, 3), (2, 3, 1)) == -5 and "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,3,1))" in err()
    assert _raw_call(osg, gpu, d, *out, (12, 7, 3), (3, 2, 1)) == -5 and "needed (halo (3,2,1))" in err()
    assert _raw_call(osg, gpu, d, *out, (12, 5, 5), (3, 3, 0)) == -5 and "needed (halo (3,3,0))" in err()
    with pytest.raises(osg._lib.TripolarHipError, match="TPG_ERR_UNSUPPORTED.*Hz >= 1 needed"):
        osg._lib.check_weno_vi(_raw_call(osg, gpu, d, *out, (12, 5, 5), (3, 3, 0)))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)
    _assert_inputs_unchanged(d, h, "refusals")


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
DT, CHI = 0.01, 0.1


@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 7), (5, 5, 5), torch.float64), ((50, 40, 3), (4, 4, 4), torch.float32)],
                         ids=["48x40x7-h5-f64", "50x40x3-h4-f32"])
def test_two_steps_eagerly_and_as_a_graph_equal_the_references_composed(osg, gpu, size, halo, tdt, immersed):
    """filled u, v and w from compute_w_from_continuity, then twice: this tendency -> ab2_velocity_step_plan(fill_halos=True).  Eagerly, Gu,
    Gv, u, v and the previous tendencies after each step are the composition of weno_vi_ref, ab2_ref and the fill's; the plan allocates
    nothing; one captured graph of the two plans replayed twice from the start gives the same arrays.  On the immersed grid the mask in the
    call is mask_immersed_field's"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v, w, Gu, Gv, Gum, Gvm = _model(osg, gpu, size, halo, tdt, immersed)
    m, dz, (nfc, ncf) = _host_metrics(osg, KERNEL, grid, tdt)
    assert (nfc is not None) == immersed and dz.shape == (Nz,)
    hw = w.data.cpu().numpy()
    tend = osg.weno_vi_momentum_advection_plan(u, v, w, Gu, Gv)
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
        assert same_bits(cut(new_u), cut(u0)) > 0 and same_bits(cut(want_Gv), cut(Gv0)) > 0
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
    if immersed:
        raw = osg.weno_vi_momentum_advection_tendency(u, v, w, mask_immersed=False)
        masked = osg.weno_vi_momentum_advection_tendency(u, v, w)
        assert all(same_bits(a.data.cpu().numpy(), b.data.cpu().numpy()) > 0 for a, b in zip(raw, masked))
        osg.mask_immersed_field(list(raw), 0)
        for a, b in zip(raw, masked):
            _assert_parent(a.data.cpu().numpy(), b.data.cpu().numpy(), "mask pass")


def test_out_is_allocated_or_given_and_filled(osg, gpu):
    """`out=None` allocates an XFaceField and a YFaceField whose halos stay zero; a given pair is written and, with fill_halos, filled; the
    one-shot call equals the plan's"""
    size, halo, tdt = (20, 12, 5), (3, 3, 1), torch.float64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v, w, Gu, Gv, _, _ = _model(osg, gpu, size, halo, tdt, False)
    m, dz, _ = _host_metrics(osg, KERNEL, grid, tdt)
    hu, hv, hw = (f.data.cpu().numpy() for f in (u, v, w))
    zero = np.zeros_like(hu)
    with np.errstate(all="ignore"):
        want = tendencies(hu, hv, hw, zero, zero, m, dz, size, halo)
    out = osg.weno_vi_momentum_advection_tendency(u, v, w)
    assert len(out) == 2 and out[0].loc == (osg.Face, osg.Center, osg.Center) and out[1].loc == (osg.Center, osg.Face, osg.Center)
    _assert_pair([o.data.cpu().numpy() for o in out], want, "allocated")
    given = osg.weno_vi_momentum_advection_tendency(u, v, w, out=(Gu, Gv), fill_halos=True)
    assert given[0] is Gu and given[1] is Gv
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    for f, x in zip((Gu, Gv), want):
        assert same_bits(f.interior().cpu().numpy().reshape(x[cut].shape)[:, :Ny - 1], x[cut][:, :Ny - 1]) == 0     # the fold may rewrite row Ny
        assert bool((f.data[Hz:Hz + Nz, Hy:Hy + Ny, :Hx] != 0).any())                                              # the halos were filled
