"""The reference of the WENO5-upwinded momentum tendency (tests/weno_momentum_ref.py) held to properties, not to itself (no GPU): a uniform
vorticity is reproduced, the two windows mirror each other, the reconstruction is fifth-order on a smooth vorticity and does not overshoot a
step, the terms it takes from momentum_ref are momentum_ref's bits, and the cells it says it reads are the cells it reads."""
import numpy as np
import pytest

import momentum_ref
import weno_momentum_ref as ref
from weno_momentum_ref import METRICS, same_bits

F32, F64 = np.float32, np.float64


def _random(size, halo, dtype, seed=0, signs=None):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, wparent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    rng = np.random.default_rng(seed)
    if signs is None:
        u, v = rng.uniform(-1, 1, parent), rng.uniform(-1, 1, parent)
    else:
        u, v = signs[0] * rng.uniform(0.5, 1, parent), signs[1] * rng.uniform(0.5, 1, parent)
    w = rng.uniform(-1, 1, wparent)
    m = {k: rng.uniform(0.5, 2, plane).astype(dtype) for k in METRICS}
    return u.astype(dtype), v.astype(dtype), w.astype(dtype), m, rng.uniform(0.5, 2, Nz + 1).astype(dtype)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_a_uniform_vorticity_is_reproduced(dtype):
    """unit metrics, v = a * i and u = b * j in small integers: Z = a - b exactly at every node of every window, so zr equals it to a few ulp
    (W5's three candidate values are (1/3 - 7/6 + 11/6) Z and the like, its indicators vanish) and hu is exactly -(vhat * zr)"""
    size, halo = (8, 6, 2), (3, 3, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, w, m, dz = _random(size, halo, dtype)
    m = {k: np.ones_like(p) for k, p in m.items()}
    a, b = 3, -2
    v = np.broadcast_to(a * np.arange(Nx + 2 * Hx, dtype=dtype)[None, None, :], v.shape).copy()
    u = np.broadcast_to(b * np.arange(Ny + 2 * Hy, dtype=dtype)[None, :, None], u.shape).copy()
    for di in range(-2, 4):
        assert (ref.zeta_at(u, v, m, size, halo, di, 0) == a - b).all() and (ref.zeta_at(u, v, m, size, halo, 0, di) == a - b).all()
    t = ref.terms(u, v, w, m, dz, size, halo)
    ulp = np.finfo(dtype).eps * abs(a - b)
    for zr in (t["zru"], t["zrv"]):
        assert np.abs(zr - dtype(a - b)).max() <= 4 * ulp          # three products, two sums and a quotient of values near Z: a few ulp
    assert same_bits(t["hu"], -(t["vhat"] * t["zru"])) == 0 and same_bits(t["hv"], t["uhat"] * t["zrv"]) == 0
    assert (t["vhat"] > 0).all() and (t["uhat"] < 0).any()         # both windows were taken


def _windows(Z, axis):
    """the six arrays Z[n-2] .. Z[n+3] along `axis` for the nodes n that have them all"""
    n = Z.shape[axis]
    return [np.take(Z, range(2 + o, n - 3 + o), axis=axis) for o in range(-2, 4)]


@pytest.mark.parametrize("axis", [0, 1], ids=["y", "x"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_the_two_windows_mirror_each_other(dtype, axis):
    """reversing the order along the axis and the sign of the transverse velocity gives the mirrored zr, bit for bit: node n of the mirrored
    field is node N - 1 - n of the original (the value is reconstructed between Z[n] and Z[n+1])"""
    rng = np.random.default_rng(3)
    Z = rng.uniform(-1, 1, (17, 19)).astype(dtype)
    vel = rng.uniform(-1, 1, (17, 19)).astype(dtype)
    vel[vel == 0] = 1
    n = Z.shape[axis]
    cut = lambda a: np.take(a, range(2, n - 3), axis=axis)         # noqa: E731
    zr = ref.upwind(cut(vel), _windows(Z, axis))
    # the mirrored problem: Z'[x] = Z[n - 1 - x]; the velocity at node x' = n - 2 - x (between Z'[x'] and Z'[x' + 1]) is minus the original's
    Zm = np.flip(Z, axis)
    velm = -np.flip(np.take(vel, range(0, n - 1), axis=axis), axis)
    velm = np.concatenate([velm, np.take(velm, [0], axis=axis)], axis=axis)        # (the last node has no window: any value)
    zrm = ref.upwind(cut(velm), _windows(Zm, axis))
    assert same_bits(np.flip(zrm, axis), zr) == 0
    assert ((cut(vel) >= 0).any() and (cut(vel) < 0).any()) and same_bits(zr, ref.upwind(-cut(vel), _windows(Z, axis))) > 0


def test_fifth_order_on_a_smooth_vorticity_and_no_overshoot_across_a_step():
    """W5 reconstructs, from the means of a smooth function over cells of width h, its value at a cell edge with an error O(h^5): over
    three resolutions the greatest error falls by more than 2^4.5 per halving (fifth order within half an order), for both windows.
    Across a step the candidate values that straddle it get weights below (1 + 1) / (tau / eps)^2 with tau of order 1 and eps = 1e-8:
    the value stays within 1e-12 of the step's range"""
    errs = {True: [], False: []}
    for N in (16, 32, 64):
        h = 2 * np.pi / N
        y = h * np.arange(-3, N + 4)                               # cell centres, three beyond either end
        mean = (np.cos(y - h / 2) - np.cos(y + h / 2)) / h         # the cell means of sin
        edge = np.sin(y[2:-3] + h / 2)                             # the edge between cell n and n + 1
        for positive in (True, False):
            vel = np.full(edge.shape, 1.0 if positive else -1.0)
            errs[positive].append(np.abs(ref.upwind(vel, _windows(mean, 0)) - edge).max())
    for e in errs.values():
        assert e[0] / e[1] > 2 ** 4.5 and e[1] / e[2] > 2 ** 4.5, e
    step = np.where(np.arange(40) < 20, 0.0, 1.0)
    for positive in (True, False):
        vel = np.full(40 - 5, 1.0 if positive else -1.0)
        zr = ref.upwind(vel, _windows(step, 0))
        assert zr.min() >= -1e-12 and zr.max() <= 1 + 1e-12 and (zr == 0).any() and (np.abs(zr - 1) < 1e-12).any()
    # ... while the same five-point value with the linear weights overshoots
    q = _windows(step, 0)
    linear = (2 * q[0] - 13 * q[1] + 47 * q[2] + 27 * q[3] - 3 * q[4]) / 60
    assert linear.max() > 1.05 or linear.min() < -0.05


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_the_vertical_and_bernoulli_terms_are_momentum_refs(dtype):
    """vu, bu, vv, bv are momentum_ref.terms' bits, Z is momentum_ref.zeta's at every shift, and Gu, Gv are the rule's last lines on them;
    only hu and hv differ from momentum_ref's"""
    size, halo = (12, 10, 4), (4, 3, 2)
    u, v, w, m, dz = _random(size, halo, dtype, 5)
    t, base = ref.terms(u, v, w, m, dz, size, halo), momentum_ref.terms(u, v, w, m, dz, size, halo)
    for k in ("vu", "bu", "vv", "bv"):
        assert same_bits(t[k], base[k]) == 0
    for k in ("hu", "hv", "Gu", "Gv"):
        assert same_bits(t[k], base[k]) > 0.9 * t[k].size
    assert same_bits(t["Gu"], -((t["hu"] + base["vu"]) + base["bu"])) == 0 and same_bits(t["Gv"], -((t["hv"] + base["vv"]) + base["bv"])) == 0
    assert same_bits(ref.zeta_at(u, v, m, size, halo, 0, 0), momentum_ref.zeta(u, v, m, size, halo)) == 0
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    big = momentum_ref.zeta(u, v, m, (Nx + 2, Ny + 2, Nz), (Hx - 1, Hy - 1, Hz))     # the same parents read as a wider interior
    assert same_bits(ref.zeta_at(u, v, m, size, halo, 1, -1), big[:, 0:Ny, 2:Nx + 2]) == 0
    G = ref.tendencies(u, v, w, np.full_like(u, 7), np.full_like(u, 7), m, dz, size, halo)
    edge = np.ones(u.shape, bool)
    edge[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
    assert all((g[edge] == 7).all() for g in G) and same_bits(G[0][~edge].reshape(t["Gu"].shape), t["Gu"]) == 0


def test_cells_read_is_what_perturbing_every_cell_finds():
    """every cell of every array of a small case scaled by 1.5, one at a time, with the transverse velocities positive everywhere and then
    negative everywhere (a window's far cell is read under one sign only): the cells whose change moves a bit of Gu or Gv are exactly
    cells_read's, and the two signs' sets differ"""
    size, halo, dtype = (4, 4, 1), (3, 3, 1), F64
    want = ref.cells_read(size, halo)
    found = {k: np.zeros(a.shape, bool) for k, a in want.items()}
    per_sign = []
    for s in (1, -1):
        u, v, w, m, dz = _random(size, halo, dtype, 9, signs=(s, s))
        arrays = dict(m, u=u, v=v, w=w)
        t = ref.terms(u, v, w, m, dz, size, halo)
        assert ((t["vhat"] >= 0) == (s > 0)).all() and ((t["uhat"] >= 0) == (s > 0)).all()
        base = (t["Gu"], t["Gv"])
        mine = {k: np.zeros(a.shape, bool) for k, a in want.items()}
        for name, a in arrays.items():
            for cell in np.ndindex(a.shape):
                keep = a[cell]
                a[cell] = keep * 1.5
                t = ref.terms(arrays["u"], arrays["v"], arrays["w"], {k: arrays[k] for k in METRICS}, dz, size, halo)
                a[cell] = keep
                mine[name][cell] = same_bits(t["Gu"], base[0]) > 0 or same_bits(t["Gv"], base[1]) > 0
        per_sign.append(mine)
        for k in found:
            found[k] |= mine[k]
    for k in want:
        assert np.array_equal(found[k], want[k]), (k, np.argwhere(found[k] != want[k])[:8])
    assert any((per_sign[0][k] != per_sign[1][k]).any() for k in ("u", "v", "dx_fc", "dy_cf", "az_ff"))
    assert not want["u"].all() and not want["az_ff"].all() and want["u"][:, 0, 3:7].any() and not want["u"][:, 0, 0].any()     # crosses, not boxes
