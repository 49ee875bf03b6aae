"""The premise of the cell kernel's column pairing (csrc/tpg_grid.hip, points_pair), checked on oracle grids without a device.

The tile kernel evaluates the latitude / atan chain of a point once for the two columns that are lambda -> -lambda images of each other,
    i' = 2 shift + 2 - i (x-Face),   i' = 2 shift + 1 - i (x-Center),   mod Nx,   shift = Nx // 4,
which is valid only if the chain gives the same bits at both.  Latitude is the chain's output that reaches an array unchanged, so the
four phi arrays must be bit-equal under the pairing on every row the fast path evaluates: y-Center rows 1..Ny-1, y-Face rows 1..Ny
(the kernel's step s = 1..Ny-1 creates the Center row s and the Face row s + 1; rows 1..Ny-1 of all four arrays are what the issue sets,
the Face row Ny is what the kernel uses on top of that).
The fold partner (Nx - i + 2 / Nx - i + 1) and i + Nx/2 pass the same check on small grids and FAIL it at Nx = 3600, where
lambda +- 180 is not representable: the last test pins that, so that nobody pairs by them."""
import numpy as np
import pytest

SHAPES = [(3600, 64), (3602, 32), (1440, 48), (62, 30)]
H = 4
_grids = {}


def _grid(oracle, Nx, Ny, dtype):
    key = (Nx, Ny, np.dtype(dtype).str)
    if key not in _grids:
        _grids[key] = oracle.build_grid((Nx, Ny, 1), halo=(H, H, 1), dtype=dtype)
    return _grids[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _image(Nx, face):
    """0-based interior column of the lambda -> -lambda image of every 0-based interior column"""
    i = np.arange(1, Nx + 1)
    ip = (2 * (Nx // 4) + (2 if face else 1) - i - 1) % Nx + 1
    return ip - 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("Nx,Ny", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_latitudes_are_bit_equal_under_the_pairing(oracle, Nx, Ny, dtype):
    g = _grid(oracle, Nx, Ny, dtype)
    for name, face_x, face_y in (("phi_cc", 0, 0), ("phi_fc", 1, 0), ("phi_cf", 0, 1), ("phi_ff", 1, 1)):
        a = g[name][H:H + Ny, H:H + Nx]                       # interior rows 1..Ny
        rows = slice(0, Ny if face_y else Ny - 1)
        own, img = _bits(a[rows]), _bits(a[rows][:, _image(Nx, face_x)])
        assert np.array_equal(own, img), (name, int((own != img).sum()))
    # the pairing is an involution; Face has exactly two fixed columns (lambda = -180 and 0), Center none
    for face in (0, 1):
        m = _image(Nx, face)
        assert np.array_equal(m[m], np.arange(Nx))
        fixed = np.flatnonzero(m == np.arange(Nx)) + 1
        assert list(fixed) == ([Nx // 4 + 1, Nx // 4 + 1 + Nx // 2] if face else [])


def test_the_other_two_symmetries_do_not_hold_at_3600(oracle):
    Nx, Ny = 3600, 64
    g = _grid(oracle, Nx, Ny, np.float64)
    i = np.arange(1, Nx + 1)
    a = g["phi_cc"][H:H + Ny - 1, H:H + Nx]
    fold = (Nx - i + 1 - 1) % Nx
    half = (i + Nx // 2 - 1) % Nx
    assert not np.array_equal(_bits(a), _bits(a[:, fold]))
    assert not np.array_equal(_bits(a), _bits(a[:, half]))
