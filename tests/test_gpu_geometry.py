"""GPU parity of the geometry utilities against the oracle: tpg_nonorthogonality_angle
(test/test_tripolar_grid.jl:8-34,49-75) and tpg_convert_frame (examples/convert_to_latlong_frame.jl:12-55).
Both sides use the same deterministic Float64 functions: bit-identical (tolerance asserted: 1e-12 absolute degrees /
1e-12 relative, as north_star states for Float64 results).

Below the first block: every kernel form of the two entry points, through the C ABI, against the oracle (bit for bit, NaNs included, on the
whole sentinel-filled destination) AND against tests/geometry_ref.py, the long-double reference written from the reference's Julia text, within
tolerances derived there from the arithmetic.  tests/test_oracle_geometry.py holds the oracle to the same reference at the same shapes."""
import functools

import numpy as np
import pytest
import torch

import geometry_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


def test_acos_device_bits(osg, oracle, gpu, tlib):
    x = np.concatenate([np.linspace(-1, 1, 4001), np.random.default_rng(1).uniform(-1, 1, 20000), [1e-20, -1e-20, 0.5, -0.5, 1.5]])
    d = torch.from_numpy(x).to(gpu)
    y = torch.empty_like(d)
    rare = torch.zeros(x.size, dtype=torch.int32, device=gpu)
    assert tlib.tpg_math_probe(10, d.data_ptr(), y.data_ptr(), rare.data_ptr(), x.size, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), oracle.math_probe("acos", x), equal_nan=True)


@pytest.mark.parametrize("size,kw", [((360, 180, 1), dict(first_pole_longitude=75, north_poles_latitude=35)),   # the reference test's grid (:52-57)
                                     ((60, 30, 1), {}), ((1440, 720, 1), {})])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_nonorthogonality_parity(osg, oracle, gpu, size, kw, dtype):
    grid = osg.TripolarGrid(osg.GPU(0), dtype, size=size, **kw)
    lam, phi = grid.interior("lambda_cc"), grid.interior("phi_cc")
    l1, pp = kw.get("first_pole_longitude", 70), kw.get("north_poles_latitude", 55)
    mask = (((lam - l1).abs() < 5) & ((pp - phi).abs() < 5)) | (((lam - (l1 + 180)).abs() < 5) & ((pp - phi).abs() < 5)) | (phi < -78)   # :59-60
    for m in (None, mask):
        got = osg.nonorthogonality_angle(grid, m).cpu().numpy()
        want = oracle.nonorthogonality_angle(grid.lambda_ff.cpu().numpy(), grid.phi_ff.cpu().numpy(), size, grid.halo_size,
                                            immersed=None if m is None else m.cpu().numpy())
        assert np.array_equal(got, want, equal_nan=True)
        assert np.nanmax(np.abs(got - want)) <= 1e-12 or np.array_equal(got, want, equal_nan=True)
    if dtype == torch.float64 and size == (360, 180, 1):
        # test/test_tripolar_grid.jl:74-75 bounds the masked range by a cubed-sphere panel's (absent: parity unpinned);
        # stated bound instead, and the diagnostic must see the singular neighbourhoods when they are not masked
        masked = osg.nonorthogonality_angle(grid, mask)
        assert float(masked.max()) < 2.0 and float(masked.min()) > -2.0


@pytest.mark.parametrize("nz,halo", [(3, (4, 4, 2)), (21, (4, 4, 4)), (5, (3, 2, 1)), (20, (5, 5, 5))], ids=["16B", "16B-21-levels", "element-aligned", "model-halo-5"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_frame_conversion_parity(osg, oracle, gpu, dtype, nz, halo):
    size = (180, 90, nz)                                                  # the example's grid (:58)
    grid = osg.TripolarGrid(osg.GPU(0), dtype, size=size, halo=halo, north_poles_latitude=35)
    u, v = osg.CenterField(grid), osg.CenterField(grid)
    rng = np.random.default_rng(9)
    ndt = np.float64 if dtype == torch.float64 else np.float32
    hu = rng.uniform(-1, 1, tuple(u.data.shape)).astype(ndt); hv = rng.uniform(-1, 1, tuple(v.data.shape)).astype(ndt)
    u.data.copy_(torch.from_numpy(hu)); v.data.copy_(torch.from_numpy(hv))
    g = {n: getattr(grid, n).cpu().numpy() for n in ("phi_cf", "phi_fc", "dy_cc", "dx_cc")}
    for to_native, fn in ((False, osg.convert_to_latlong_frame), (True, osg.convert_to_native_frame)):
        uo, vo = fn(grid, u, v)
        wu, wv = oracle.convert_frame(g, hu, hv, size, halo, to_native=to_native)
        assert np.array_equal(uo.data.cpu().numpy(), wu) and np.array_equal(vo.data.cpu().numpy(), wv), to_native
    # the example's use (:61-83): a purely zonal unit flow, converted and converted back
    one, zero = osg.CenterField(grid), osg.CenterField(grid)
    one.set_(1)
    utr, vtr = osg.convert_to_latlong_frame(grid, one, zero)
    ub, vb = osg.convert_to_native_frame(grid, utr, vtr)
    tol = 1e-13 if dtype == torch.float64 else 1e-5
    assert float((ub.interior() - 1).abs().max()) < tol and float(vb.interior().abs().max()) < tol


def test_geometry_argument_errors(osg, gpu):
    lib = osg._lib.lib()
    assert lib.tpg_nonorthogonality_angle(None, None, None, None, 60, 30, 4, 4, 1, None) == -1
    assert lib.tpg_nonorthogonality_angle(1 << 20, 1 << 20, None, 1 << 20, 61, 30, 4, 4, 1, None) == -2      # odd Nlambda
    assert lib.tpg_convert_frame(*([1 << 20] * 8), 0, 60, 30, 1, 0, 4, 0, 1, None) == -5                    # needs i+1 / j+1 halos


# ---- every kernel form, through the C entry points ---------------------------------------------------------------------------------------


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _dev(host, gpu, offset=0):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return t


@functools.lru_cache(maxsize=None)
def _grid(oracle, nx, ny, halo, dtype):
    """the grid arrays of one geometry, built once on the host and shared (read-only) by the cases that use it"""
    return oracle.build_grid((nx, ny, 1), dtype=dtype, halo=halo)


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _angle(osg, gpu, lam, phi, mask, size, halo, dtype):
    """one call of tpg_nonorthogonality_angle into a sentinel-filled buffer with a guard element on either side -> (Ny, Nx) host array"""
    (Nx, Ny), (Hx, Hy) = size, halo
    raw = torch.full((Nx * Ny + 2,), SENTINEL, dtype=torch.float64, device=gpu)
    osg._lib.check(osg._lib.lib().tpg_nonorthogonality_angle(lam.data_ptr(), phi.data_ptr(), None if mask is None else mask.data_ptr(),
                                                             raw.data_ptr() + 8, Nx, Ny, Hx, Hy, osg._lib.ft_of(_tdt(dtype)),
                                                             osg._lib.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    out = raw.cpu().numpy()
    assert out[0] == SENTINEL and out[-1] == SENTINEL, "a guard element was written"
    got = out[1:-1].reshape(Ny, Nx)
    assert not (_bits(got) == _bits(np.float64(SENTINEL))).any(), "an element of angle was not written"
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("halo", R.ANGLE_HALOS, ids=lambda h: "h%d%d%d" % h)
@pytest.mark.parametrize("size", R.ANGLE_SIZES, ids=lambda s: "%dx%d" % s)
def test_angle_at_tile_edges(osg, oracle, gpu, size, halo, dtype):
    """Nx, Ny on both sides of the kernel's tile edges (63 x 7 cells per block of 64 x 8 nodes), four halos, with and without a mask (a byte
    plane at an odd address): equal to the oracle bit for bit, within tolerance of the long-double reference on every valid node, every
    element of the destination written and nothing around it"""
    g = _grid(oracle, *size, halo, dtype)
    lam, phi = _dev(g["lambda_ff"], gpu), _dev(g["phi_ff"], gpu)
    for mask in (None, R.angle_mask(size)):
        dm = None if mask is None else _dev(mask, gpu, 1)
        assert dm is None or dm.data_ptr() % 2 == 1
        got = _angle(osg, gpu, lam, phi, dm, size, halo[:2], dtype)
        want = oracle.nonorthogonality_angle(g["lambda_ff"], g["phi_ff"], (*size, 1), halo, immersed=mask)
        assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:4]
        ref, tol, valid = R.angle_ref(g["lambda_ff"], g["phi_ff"], (*size, 1), halo, immersed=mask)
        excluded = ~valid | np.isnan(want)
        assert np.array_equal(excluded, ~valid) and excluded.sum() <= 0.01 * (size[0] - 1) * (size[1] - 1), excluded.sum()
        err = np.abs(got - ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.max(np.where(valid & (tol > 0), err / tol, 0)))
        assert np.all(err[valid] <= tol[valid]), f"worst error / tol = {ratio:.3f}"
        assert ratio < 1, ratio


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_angle_reads_no_halo_cell(osg, oracle, gpu, dtype):
    """the C entry point with Hx = Hy = 0 on the dense interior of lambda_ff / phi_ff, and the padded call with every halo cell poisoned:
    both equal the padded call bit for bit (the launch over (Nx-1, Ny-1) reads nodes (1..Nx, 1..Ny) only)"""
    size, halo = (130, 36), (5, 5, 5)
    (Nx, Ny), (Hx, Hy, _) = size, halo
    g = _grid(oracle, *size, halo, dtype)
    mask = _dev(R.angle_mask(size), gpu, 1)
    padded = _angle(osg, gpu, _dev(g["lambda_ff"], gpu), _dev(g["phi_ff"], gpu), mask, size, (Hx, Hy), dtype)
    inner = (slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    dense = _angle(osg, gpu, _dev(g["lambda_ff"][inner], gpu), _dev(g["phi_ff"][inner], gpu), mask, size, (0, 0), dtype)
    assert np.array_equal(_bits(dense), _bits(padded))
    poisoned = []
    for name in ("lambda_ff", "phi_ff"):
        a = np.full_like(g[name], np.nan)
        a[inner] = g[name][inner]
        poisoned.append(_dev(a, gpu))
    assert np.array_equal(_bits(_angle(osg, gpu, *poisoned, mask, size, (Hx, Hy), dtype)), _bits(padded))
    assert np.isfinite(padded).all()


FRAME_CASES = [(geom, nz) for geom in R.FRAME_GEOMS for nz in R.frame_levels(geom)]
FRAME_OFFSETS = [(0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 1, 0)]      # elements past an allocation: u, v, u_out, v_out


def _frame_form(nx, hx, dtype, offsets):
    """the kernel tpg_convert_frame launches (csrc/tpg_geometry.hip), from the geometry and the pointers' offsets past 16-B-aligned allocations"""
    W = 16 // np.dtype(dtype).itemsize
    if nx % W:
        return "scalar"
    return "vec" if hx % W == 0 and not any(offsets) else "loose"


def test_frame_cases_reach_every_kernel_form():
    forms = {(np.dtype(dt).name, _frame_form(geom[0][0], geom[1][0], dt, off), "pointer" if any(off) else "halo")
             for geom, _ in FRAME_CASES for dt in (np.float32, np.float64) for off in FRAME_OFFSETS}
    assert {("float32", "scalar", "halo"), ("float32", "scalar", "pointer"), ("float32", "vec", "halo"), ("float64", "vec", "halo"),
            ("float32", "loose", "halo"), ("float64", "loose", "halo"), ("float32", "loose", "pointer"), ("float64", "loose", "pointer")} <= forms
    assert ("float64", "scalar", "halo") not in forms                # Nx is even: Float64 rows always split into 16-B chunks
    # a single misaligned pointer leaves the aligned form, at a halo that would otherwise keep it
    assert _frame_form(64, 4, np.float32, (0, 0, 1, 0)) == "loose" and ((64, 12), (4, 4, 2)) in R.FRAME_GEOMS


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("geom,nz", FRAME_CASES, ids=lambda c: "%dx%d-h%d%d%d" % (*c[0], *c[1]) if isinstance(c, tuple) else "nz%d" % c)
def test_frame_rotation_every_form(osg, oracle, gpu, geom, nz, dtype):
    """tpg_convert_frame through the C ABI into sentinel-filled parents, both directions, at three placements of the four field pointers:
    the WHOLE parent equals the oracle's interior in the sentinel frame (as integers), the interior is within 16 eps (|u| + |v|) of the
    long-double reference, and the non-finite cells are the reference's (the pole cells: two per level, only when Nx = 2 mod 4)"""
    (nx, ny), halo = geom
    size = (nx, ny, nz)
    lib, ft, stream = osg._lib.lib(), osg._lib.ft_of(_tdt(dtype)), osg._lib.current_stream_ptr(gpu)
    g = _grid(oracle, nx, ny, halo, dtype)
    dg = [_dev(g[n], gpu) for n in ("phi_cf", "phi_fc", "dy_cc", "dx_cc")]
    u, v = R.frame_inputs(size, halo, dtype)
    I = tuple(slice(h, h + n) for h, n in zip(halo[::-1], size[::-1]))
    worst = 0.0
    for to_native in (False, True):
        wants = oracle.convert_frame(g, u, v, size, halo, to_native=to_native)
        *refs, scale = R.frame_ref(g, u, v, size, halo, to_native)
        tol = R.frame_tolerance(scale, dtype)
        fins = [np.isfinite(r) for r in refs]
        for fin in fins:
            assert (~fin).reshape(nz, -1).sum(1).max() <= (2 if nx % 4 == 2 else 0)
        for offsets in FRAME_OFFSETS:
            du, dv = _dev(u, gpu, offsets[0]), _dev(v, gpu, offsets[1])
            raws = [torch.full((u.size + o,), SENTINEL, dtype=_tdt(dtype), device=gpu) for o in offsets[2:]]
            outs = [r[o:].view(u.shape) for r, o in zip(raws, offsets[2:])]
            assert all((t.data_ptr() % 16 != 0) == bool(o) for t, o in zip((du, dv, *outs), offsets))
            osg._lib.check(lib.tpg_convert_frame(*(a.data_ptr() for a in dg), du.data_ptr(), dv.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                 int(to_native), nx, ny, nz, *halo, ft, stream))
            torch.cuda.synchronize()
            for raw, o, want, ref, fin in zip(raws, offsets[2:], wants, refs, fins):
                whole = raw.cpu().numpy()
                assert o == 0 or whole[0] == SENTINEL, "the element in front of an offset parent was written"
                got = whole[o:].reshape(u.shape)
                expect = np.full(u.shape, SENTINEL, dtype=dtype)
                expect[I] = want[I]
                assert np.array_equal(_bits(got), _bits(expect)), (to_native, offsets, np.argwhere(_bits(got) != _bits(expect))[:4])
                assert np.array_equal(np.isnan(got[I]), np.isnan(ref)) and np.array_equal(np.isfinite(got[I]), fin), (to_native, offsets)
                err = np.abs(got[I][fin] - ref[fin])
                worst = max(worst, float(np.max(err / tol[fin])))
                assert np.all(err <= tol[fin]), f"worst error / tol = {worst:.3f} (to_native = {to_native}, offsets = {offsets})"
    assert worst < 1, worst


def test_public_conversion_on_a_float32_grid_with_nx_2_mod_4(osg, oracle, gpu):
    """convert_to_latlong_frame / convert_to_native_frame on a Float32 grid with Nx = 90: rows do not split into chunks of 4, so this is the
    scalar kernel; equal to the oracle on the whole parent, NaN at the two pole cells of every level (dx_cc = 0) and nowhere else"""
    size, halo = (90, 45, 5), (4, 4, 4)
    assert size[0] % 4 == 2 and _frame_form(size[0], halo[0], np.float32, (0, 0, 0, 0)) == "scalar"
    grid = osg.TripolarGrid(osg.GPU(0), torch.float32, size=size, halo=halo)
    u, v = osg.CenterField(grid), osg.CenterField(grid)
    hu, hv = R.frame_inputs(size, halo, np.float32)
    u.data.copy_(torch.from_numpy(hu)); v.data.copy_(torch.from_numpy(hv))
    g = {n: getattr(grid, n).cpu().numpy() for n in ("phi_cf", "phi_fc", "dy_cc", "dx_cc")}
    I = tuple(slice(h, h + n) for h, n in zip(halo[::-1], size[::-1]))
    pole = np.broadcast_to(g["dx_cc"][I[1:]] == 0, (size[2], size[1], size[0]))
    assert np.argwhere(pole[0]).tolist() == [[44, 44], [44, 45]]
    for to_native, fn in ((False, osg.convert_to_latlong_frame), (True, osg.convert_to_native_frame)):
        outs = fn(grid, u, v)
        wants = oracle.convert_frame(g, hu, hv, size, halo, to_native=to_native)
        *refs, scale = R.frame_ref(g, hu, hv, size, halo, to_native)
        for o, want, ref in zip(outs, wants, refs):
            got = o.data.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), to_native
            assert np.array_equal(np.isnan(got[I]), pole) and np.array_equal(~np.isfinite(ref), pole)
            assert np.all(np.abs(got[I][~pole] - ref[~pole]) <= R.frame_tolerance(scale, np.float32)[~pole])
