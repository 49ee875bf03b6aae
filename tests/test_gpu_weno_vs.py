"""GPU tests of the momentum advection tendency of the drivers' scheme, WENOVectorInvariant(vorticity_order = 5):
tpg_weno_vs_momentum_advection_tendency through the C ABI, and weno_vs_momentum_advection_tendency / weno_vs_momentum_advection_plan through
the package.  Compared BIT FOR BIT with tests/weno_vs_ref.py (numpy in the fields' type: every operation of the rule is one correctly rounded
IEEE operation, so the reference is exact and there is no tolerance anywhere in this file); NaNs compare by NaN-ness; whole parents are
compared: the halo cells of Gu, Gv against a sentinel, and the inputs must come back unchanged.  Inputs are random in every cell, dz_c and
the metrics in [0.5, 2].  tests/test_weno_vs_ref.py holds, on the CPU, that on every case drawn here hu and hv differ in bits from the
DefaultStencil ones: a call that launched the DefaultStencil form would fail every comparison below.

Only the first launch is new; the second (k_weno_vi_finish) is tests/test_gpu_weno_vi.py's.  Shapes, the smallest at which each path of the
first launch can go wrong:
- 12 x 5 x 2 in the three chunk forms (halo 4 on the 16-B grid; the same with every pointer one element off it; halo (3, 3, 1): an odd Hx),
  Float32 and Float64.  Ny = 5 is odd: two rows per item, the last tile is partial.  12 x 5 x 9 once more through every class of the finish.
- (4, 3, 1) at halo (3, 3, 1) and (4, 4, 5) at halo (4, 4, 4): the smallest served; 10 x 5 x 6 in Float32: 8-B chunks (Nx = 2 mod 4).
- 130 x 4 x 2 in Float64 and 260 x 4 x 2 in Float32: 65 chunks a row, so a wave edge (64 | 65), a row end and the periodic seam fall inside
  the arms: there a lane forms the Z beside its chunk itself, next to the UB and VB it forms from element loads (ub_at, vb_at) everywhere.
Not here: a case past 2^31 elements.  The offsets are the shared template's, held by tests/test_gpu_tendency_edges.py; ub_at and vb_at use
the 64-bit `ro[] + c` arithmetic of zeta_at and read exactly its elements of u and v."""
import numpy as np
import pytest
import torch

import ab2_ref
import gpu_harness as H
import tendency_windows as tw
import weno_vs_ref
from gpu_harness import (F32, F64, MASK_VALUE, SENTINEL, _assert_inputs_unchanged, _assert_pair, _assert_parent, _count_planes, _dev,  # noqa: F401
                         _filled, _free_hbm, _host_metrics, _velocity_model as _model)
from special_values import pool
from weno_vs_ref import METRICS, cells_read, same_bits, tendencies, terms

pytestmark = pytest.mark.gpu

# jt: the rows per item the library is built with (TPG_WVS_JT, TPG_WVS_JT_F32 of csrc/tpg_weno_vs.hip)
KERNEL = tw.Kernel("weno_vs", "weno_vs", "tpg_weno_vs_momentum_advection_tendency", arm=(3, 3, 1), centred_in_z=False, scheme_arg=False,
                   jt={8: 2, 4: 2}, share=False, ref=tw._momentum_ref(weno_vs_ref, tw._UPWINDED), **tw._UPWINDED)
FORMS = {"aligned": ((4, 4, 4), 0), "offset": ((4, 4, 4), 1), "oddHx": ((3, 3, 1), 0)}
LAUNCH1 = [(((12, 5, 2), halo, dtype), off, f"12x5x2-{form}-{'f64' if dtype == F64 else 'f32'}")
           for form, (halo, off) in FORMS.items() for dtype in (F64, F32)]
FINISH = [(((12, 5, 9), (4, 4, 4), F64), 0, "12x5x9-aligned-f64"), (((12, 5, 9), (3, 3, 1), F32), 0, "12x5x9-oddHx-f32")]
SMALL = [(((4, 3, 1), (3, 3, 1), F64), 0, "4x3x1-h331-f64"), (((4, 3, 1), (3, 3, 1), F32), 0, "4x3x1-h331-f32"),
         (((4, 4, 5), (4, 4, 4), F64), 0, "4x4x5-h444-f64"), (((4, 4, 5), (4, 4, 4), F32), 0, "4x4x5-h444-f32"),
         (((10, 5, 6), (4, 4, 4), F32), 0, "10x5x6-h444-f32-8B")]
EDGES = [(((130, 4, 2), (4, 4, 4), F64), 0, "130x4x2-h444-f64"), (((130, 4, 2), (3, 3, 1), F64), 0, "130x4x2-h331-f64"),
         (((260, 4, 2), (4, 4, 4), F32), 0, "260x4x2-h444-f32")]
ALL = LAUNCH1 + FINISH + SMALL + EDGES
SOME = EDGES + [c for c in ALL if c[2] in ("12x5x2-offset-f64", "10x5x6-h444-f32-8B")]
BIGGER = [(((48, 40, 9), (5, 5, 5), F64), 0, "48x40x9-h5-f64"), (((48, 40, 9), (4, 4, 4), F32), 0, "48x40x9-h4-f32")]
SELECT = [((12, 9, 3), (3, 3, 1), F64), ((12, 9, 3), (3, 3, 1), F32)]
BANDS = ((40, 24, 3), {F64: (4, 4, 4), F32: (3, 3, 1)})
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
    """tpg_weno_vs_momentum_advection_tendency on the device arrays d into fresh sentinel-filled outputs -> the whole parents (Gu, Gv) on the host"""
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
    """every cell of u, v, w and the eight metric planes that the rule does not read (weno_vi_ref.cells_read: the new smoothness inputs read
    no cell more) is NaN: the result has no NaN and equals the clean one.  On the wave-edge cases this covers ub_at and vb_at"""
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


@_params(SOME)
def test_fused_mask_equals_the_reference(osg, gpu, case, offset):
    """with the count planes: the reference with the mask, bit for bit on the whole parents; the masked and the unmasked reference differ"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    nfc, ncf = _count_planes(case, varied=False)
    want = _ref(h, size, halo, nfc, ncf)
    assert same_bits(want[0], h["want"][0]) > 0 and same_bits(want[1], h["want"][1]) > 0
    d = _device(h, gpu, offset)
    nd = [_dev(nfc, gpu, offset), _dev(ncf, gpu, offset)]
    _assert_pair(_call(osg, gpu, d, size, halo, n_fc=nd[0], n_cf=nd[1], value=MASK_VALUE, offset=offset), want, "fused mask")


def _planted(case):
    """the case with +-0, subnormals, +-Inf, NaN, +-max planted in 0.5 % of the cells of u and v"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _case(case)
    rng = np.random.default_rng([7, *size, *halo])
    p = pool(dtype)
    planted = {k: h[k] for k in SHARED}
    for name in ("u", "v"):
        a = h[name].copy()
        where = rng.random(a.shape) < 0.005
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
        planted[name] = a
    # whatever the draw gave: a NaN, an Inf and a -0 velocity cell in the interior
    planted["u"][Hz, Hy + 1, Hx + 1], planted["v"][Hz, Hy + 3, Hx + 3], planted["u"][Hz, Hy + 2, Hx + 3] = np.nan, np.inf, -0.0
    return planted


@_params(BIGGER)
def test_special_values_in_read_cells(osg, gpu, case, offset):
    """+-0, subnormals, +-Inf, NaN, +-max planted in read cells of u and v, which now also arrive through UB and VB: bit for bit numpy's,
    which computes the same IEEE operations.  The reference's interior stays more than 20 % finite with NaN in it -- asserted before
    comparing.  48 x 40: the model halo 5, more than one block"""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    planted = _planted(case)
    want = _ref(planted, size, halo)
    for G in want:
        inner = G[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(inner).any() and np.isfinite(inner).mean() > 0.2
    _assert_pair(_call(osg, gpu, _device(planted, gpu, offset), size, halo, offset=offset), want, "special values")


@pytest.mark.parametrize("case", SELECT, ids=["f64", "f32"])
def test_selection_at_minus_zero_and_nan(osg, gpu, case):
    """`vhat >= 0`, `uhat >= 0` are true for -0 and false for NaN.
    - v = -0 everywhere: vhat is -0 at every node (asserted) and hu = -(vhat * zr) is +-0 -- unless zr is not finite.  u carries an Inf in
      one row, which the right-biased window of the row three south of it holds and the left-biased one does not: the NaNs of the
      reference there are those of the LEFT-biased window, a choice by the sign bit would give others (asserted on the reference with
      v = -tiny).  The same for u = -0 and uhat.
    - NaN planted in u and v: vhat, uhat are NaN around it, the right-biased window is taken; only NaN-ness is observable there."""
    size, halo, dtype = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    base = _case(case)
    m = {k: base[k] for k in METRICS}
    for zeroed, other, key, hkey in (("v", "u", "vhat", "hu"), ("u", "v", "uhat", "hv")):
        h = dict(base)
        h[zeroed] = np.full_like(base[zeroed], -0.0)
        a = base[other].copy()
        if other == "u":
            a[:, Hy + 6, :] = np.inf                               # UB[., j = 7 and 8]: in the windows j-1..j+3 of the rows 4..9 only
        else:
            a[:, :, Hx + 8] = np.inf
        h[other] = a
        t = terms(h["u"], h["v"], h["w"], m, h["dz_c"], size, halo)
        assert (t[key] == 0).all() and np.signbit(t[key]).all()
        tiny = dict(h)
        tiny[zeroed] = np.full_like(base[zeroed], -1e-30)
        t2 = terms(tiny["u"], tiny["v"], tiny["w"], m, h["dz_c"], size, halo)
        assert (np.isnan(t[hkey]) != np.isnan(t2[hkey])).any()
        _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), _ref(h, size, halo), ("minus zero", zeroed))
    for name in ("u", "v"):
        h = dict(base)
        h[name] = base[name].copy()
        h[name][Hz + 1, Hy + 4, Hx + 5] = np.nan
        want = _ref(h, size, halo)
        assert all(0 < np.isnan(G).sum() < 400 for G in want)
        _assert_pair(_call(osg, gpu, _device(h, gpu), size, halo), want, ("nan", name))


@pytest.mark.parametrize("layout", ["three", "thin"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_latitude_bands_equal_the_global_field(osg, gpu, dtype, layout):
    """40 x 24 x 3 cut into bands as rows jstart - Hy .. jend + Hy of every array: three bands of 8 rows, and a band of exactly Hy rows
    beside one of Hy + 1 rows and the rest.  Each band's output equals, as a whole parent, the reference on the cut, and its interior the
    matching rows of the global DEVICE result"""
    size, halo = BANDS[0], BANDS[1][dtype]
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = {k: a for k, a in tw.draw(KERNEL, size, halo, dtype).items()}
    glob = H._run(osg, gpu, KERNEL, h, size, halo, True)
    want = KERNEL.ref(h, size, halo, True)
    for name in KERNEL.outputs:
        _assert_parent(glob[name], want[name], ("global", name))
    bands = tw.band_layouts(Ny, Hy)[layout]
    assert sum(rows for _, rows in bands) == Ny and (layout != "thin" or (bands[0][1], bands[1][1]) == (Hy, Hy + 1))
    for lo, rows in bands:
        cut, bsize = tw.row_cut(KERNEL, h, size, halo, lo, rows)
        got = H._run(osg, gpu, KERNEL, cut, bsize, halo, True)
        ref = KERNEL.ref(cut, bsize, halo, True)
        for name in KERNEL.outputs:
            _assert_parent(got[name], ref[name], ("band parent", name, lo, rows))
            g, w = tw.interior(KERNEL, got[name], bsize, halo), tw.interior(KERNEL, glob[name], size, halo)[..., lo:lo + rows, :]
            assert same_bits(g, w) == 0, ("band against global", name, lo, rows)


def test_error_returns_on_device_pointers(osg, gpu):
    """refusals with real device arrays: nothing is launched -- neither launch --, the outputs keep the sentinel"""
    case = ((12, 5, 3), (3, 3, 1), F64)
    size, halo, dtype = case
    h = _case(case)
    d = _device(h, gpu)
    lib = osg._lib.weno_vs_lib()
    err = lambda: lib.tpg_weno_vs_last_error().decode()           # noqa: E731
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
        osg._lib.check_weno_vs(_raw_call(osg, gpu, d, *out, (12, 5, 5), (3, 3, 0)))
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in out)
    _assert_inputs_unchanged(d, h, "refusals")


# ---- the package ---------------------------------------------------------------------------------------------------------------------------
DT, CHI = 0.01, 0.1


@pytest.mark.parametrize("immersed", [False, True], ids=["tripolar", "immersed"])
def test_a_step_eagerly_and_as_a_graph_equals_the_references_composed(osg, gpu, immersed):
    """48 x 40 x 7 at halo 5: filled u, v and w from compute_w_from_continuity, then this tendency -> ab2_velocity_step_plan(fill_halos=True).
    Eagerly, Gu, Gv, u, v and the previous tendencies are the composition of weno_vs_ref, ab2_ref and the fill's; the plan allocates
    nothing; one captured graph of the two plans replayed from the start gives the same arrays.  On the immersed grid the mask in the call
    is mask_immersed_field's"""
    from orthogonalsphericalshellgrids.jl_amd import weno_vs
    size, halo, tdt = (48, 40, 7), (5, 5, 5), torch.float64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid, u, v, w, Gu, Gv, Gum, Gvm = _model(osg, gpu, size, halo, tdt, immersed)
    m, dz, (nfc, ncf) = _host_metrics(osg, KERNEL, grid, tdt)
    assert (nfc is not None) == immersed and dz.shape == (Nz,)
    hw = w.data.cpu().numpy()
    tend = osg.weno_vs_momentum_advection_plan(u, v, w, Gu, Gv, scheme=weno_vs.BUILT)
    step = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gum, Gvm, DT, chi=CHI, fill_halos=True)
    everything = [u, v, Gu, Gv, Gum, Gvm]
    start = [f.data.clone() for f in everything]
    cut = lambda a: a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]          # noqa: E731
    u0, v0, Gu0, Gv0, Gum0, Gvm0 = (f.data.cpu().numpy() for f in everything)
    assert tend() is tend and step() is step
    with np.errstate(all="ignore"):
        want_Gu, want_Gv = tendencies(u0, v0, hw, Gu0, Gv0, m, dz, size, halo, nfc, ncf, 0.0)
    new_u, prev_u, _ = ab2_ref.ab2_step(u0, want_Gu, Gum0, DT, CHI, ab2_ref.STORE, size, halo)
    new_v, prev_v, _ = ab2_ref.ab2_step(v0, want_Gv, Gvm0, DT, CHI, ab2_ref.STORE, size, halo)
    new_u, new_v = _filled(osg, u, cut(new_u), u0, u.boundary_conditions), _filled(osg, v, cut(new_v), v0, v.boundary_conditions)
    for name, f, x in zip(("u", "v", "Gu", "Gv", "Gum", "Gvm"), everything, [new_u, new_v, want_Gu, want_Gv, prev_u, prev_v]):
        _assert_parent(f.data.cpu().numpy(), x, name)
    eager = [f.data.clone() for f in everything]
    for f, t in zip(everything, start):
        f.data.copy_(t)
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
    torch.cuda.synchronize()
    for f, t in zip(everything, eager):
        _assert_parent(f.data.cpu().numpy(), t.cpu().numpy(), "a replay against an eager step")
    _assert_parent(w.data.cpu().numpy(), hw, "w unchanged")
    if immersed:
        raw = osg.weno_vs_momentum_advection_tendency(u, v, w, mask_immersed=False)
        masked = osg.weno_vs_momentum_advection_tendency(u, v, w)
        assert all(same_bits(a.data.cpu().numpy(), b.data.cpu().numpy()) > 0 for a, b in zip(raw, masked))
        osg.mask_immersed_field(list(raw), 0)
        for a, b in zip(raw, masked):
            _assert_parent(a.data.cpu().numpy(), b.data.cpu().numpy(), "mask pass")
