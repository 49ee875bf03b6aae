"""The paired cell kernel (k_cells_tile: each lambda -> -lambda column pair's point chains evaluated once per wave, csrc/tpg_grid.hip)
against the oracle, bit for bit, all 20 arrays, Float64 and Float32, through the product entry point (TripolarGrid -> tpg_build_grid).
Shapes are the smallest at which the pairing's layout takes another path: one tile per row, a partial last tile, Nx = 2 (mod 4), halves
shorter than a strip (aprons wrap more than once), the flagship's column geometry as thin bands (which also put the general rows 0 / Ny
and fast rows into one tile), and the first_pole_longitude values that change the longitude chain or switch the fast path off.
The full sizes are tests/test_gpu_grid.py's; variant 2 against 0 is tests/test_gpu_variants.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H4, H5 = (4, 4, 4), (5, 5, 5)
# (size, halo, extra keywords, band (jstart, jend) or None)
CASES = [
    ((60, 30, 1), H4, {}, None),                                   # exactly one tile per row
    ((62, 30, 1), H4, {}, None),                                   # Nx = 2 (mod 4), partial second tile
    ((124, 40, 1), H4, {}, None),                                  # three tiles, the last one partial
    ((4, 12, 1), H4, {}, None),                                    # smallest even Nx at halo 4: halves shorter than a strip, aprons wrap
    ((3602, 40, 1), H4, {}, None),
    ((3600, 1800, 1), H4, {}, (1, 12)),                            # the flagship's columns; row 0 general + fast rows in one tile
    ((3600, 1800, 1), H4, {}, (1789, 1800)),                       # ... row Ny general + fast rows
    ((3600, 1800, 1), H5, {}, (1, 12)),
    ((3600, 1800, 1), H5, {}, (1789, 1800)),
    ((124, 40, 1), H4, dict(first_pole_longitude=-90), None),      # fplp90 = 0
    ((124, 40, 1), H4, dict(first_pole_longitude=70), None),
    ((124, 40, 1), H4, dict(first_pole_longitude=300), None),      # |fplp90| > 360: no row takes the fast path
]


def _id(case):
    size, halo, kw, band = case
    s = f"{size[0]}x{size[1]}-h{halo[0]}"
    if band:
        s += f"-rows{band[0]}to{band[1]}"
    if kw:
        s += f"-fpl{kw['first_pole_longitude']}"
    return s


_ref = {}


def _reference(oracle, case, dtype):
    """the oracle's arrays of a case: computed once, shared, left unchanged.  The oracle evaluates the whole globe whatever the band,
    so the band cases of one (size, halo, dtype) are cut out of ONE global build (rows jstart - Hy .. jend + Hy, as
    tests/test_gpu_grid.py's band tests do) and the globe is dropped"""
    size, halo, kw, band = case
    key = (_id(case), np.dtype(dtype).str)
    if key not in _ref:
        if band:
            oracle.set_threads(min(16, oracle.max_threads()))
            glob = oracle.build_grid(size, dtype=dtype, halo=halo, **kw)
            oracle.set_threads(1)
            for other in CASES:
                if other[3] and other[:3] == case[:3]:
                    j0, j1 = other[3]
                    _ref[(_id(other), key[1])] = {n: a[j0 - 1:j1 + 2 * halo[1]].copy() for n, a in glob.items()}
            del glob
        else:
            _ref[key] = oracle.build_grid(size, dtype=dtype, halo=halo, **kw)
    for a in _ref[key].values():
        a.setflags(write=False)
    return _ref[key]


def _build(osg, case, tdt):
    size, halo, kw, band = case
    arch = osg.GPU(0)
    if band:
        j0, j1 = band
        sizes = (j1, size[1] - j1) if j0 == 1 else (j0 - 1, j1 - j0 + 1)
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=2, y_sizes=sizes), local_rank=0 if j0 == 1 else 1)
    g = osg.TripolarGrid(arch, tdt, size=size, halo=halo, **kw)
    if band:
        assert g.jrange == band
    return g


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_twenty_arrays_equal_the_oracle_bit_for_bit(osg, oracle, gpu, case, dtype):
    ref = _reference(oracle, case, dtype)
    g = _build(osg, case, torch.float64 if dtype == np.float64 else torch.float32)
    assert len(ref) == 20
    for name, r in ref.items():
        got = getattr(g, name).cpu().numpy()
        assert got.shape == r.shape and got.dtype == r.dtype, name
        same = _bits(got) == _bits(r)
        assert same.all(), (name, int((~same).sum()), np.argwhere(~same)[:4].tolist())
    # The two self-paired Face columns, named: lambda = -180 and lambda = 0 (stored columns shift + 1 and shift + 1 + Nx/2) are their
    # own images and x = -+0 there, so the lane that receives atan(y / x) must give it the sign of its own y / x, not the negated one
    (Nx, _, _), (Hx, _, _) = case[0], case[1]
    for i in (Nx // 4 + 1, Nx // 4 + 1 + Nx // 2):
        for name in ("lambda_fc", "lambda_ff"):
            got = getattr(g, name).cpu().numpy()[:, i + Hx - 1]
            assert np.array_equal(_bits(got), _bits(ref[name][:, i + Hx - 1])), (name, i)
