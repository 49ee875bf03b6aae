"""Argument-by-argument bit identity of the deterministic Float64 math:
  (a) device scalar functions (csrc/tpg_math.hpp)  ==  oracle functions (oracle/detmath.h);
  (b) device batch forms (csrc/tpg_batch.hpp)      ==  device scalar functions on their fast domain,
      with the `rare` flag raised exactly outside it.
This is what makes the GPU grid bit-identical to the CPU restatement by construction."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 400_000
SCALAR = {"sin": 0, "cos": 1, "sind": 2, "cosd": 3, "tand": 4, "atan": 5, "asin": 6, "asinh": 7, "sinh": 8, "cosh": 9,
          "acos": 10}                               # F_ACOS (csrc/tpg_probe.hip): acosD, used by the non-orthogonality angle kernel
SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 45.0, -45.0, 90.0, -90.0, 135.0, 180.0, -180.0, 225.0, 270.0, 315.0,
                    359.99999999999994, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -27, 2.0 ** -26, 2.0 ** 66, 1e300,
                    np.inf, -np.inf, np.pi / 4, -np.pi / 4, np.nextafter(np.pi / 4, 1), np.pi / 2, np.pi, -np.pi,
                    np.nextafter(np.pi, 0), 0.975, 0.9999999999999999, 5e-324, 1e-310])


def probe(osg, gpu, which, x):
    from tools import testlib                     # tpg_math_probe is a test-library hook (include/tripolar_hip_test.h)
    lib = testlib.lib()
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(gpu)
    yd = torch.empty_like(xd)
    rd = torch.zeros(xd.numel(), dtype=torch.int32, device=gpu)
    assert lib.tpg_math_probe(which, xd.data_ptr(), yd.data_ptr(), rd.data_ptr(), xd.numel(), None) == 0
    torch.cuda.synchronize()
    return yd.cpu().numpy(), rd.cpu().numpy().astype(bool)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def args_for(name, rng):
    u = rng.uniform
    parts = {
        "sin": [u(-4, 4, N), np.pi + u(-1e-6, 1e-6, 2000), u(-1e-3, 1e-3, N // 4), 10.0 ** u(-300, -5, 2000)],
        "cos": [u(-4, 4, N), np.pi / 2 + u(-1e-9, 1e-9, 2000), u(-1e-3, 1e-3, N // 4)],
        "sind": [u(-400, 400, N), np.arange(-720, 721, 15.0), u(-1e-9, 1e-9, 2000)],
        "cosd": [u(-400, 400, N), np.arange(-720, 721, 15.0), 90 + u(-1e-9, 1e-9, 2000)],
        "tand": [u(0, 89, N // 2)],
        "atan": [u(-5, 5, N), 10.0 ** u(-40, 40, N // 4) * rng.choice([-1, 1], N // 4)],
        "asin": [u(-1, 1, N), 10.0 ** u(-30, 0, N // 4), 1 - 10.0 ** u(-16, -1, 5000)],
        "acos": [u(-1, 1, N), 1 - 10.0 ** u(-16, -1, 5000), -(1 - 10.0 ** u(-16, -1, 5000)), np.array([1.0, -1.0, 0.5, -0.5, 0.0])],
        "asinh": [u(0, 40, 20000), 10.0 ** u(-12, 1, 20000)],
        "sinh": [u(0, 6, 20000), 10.0 ** u(-12, 0, 20000)],
        "cosh": [u(0, 6, 20000), 10.0 ** u(-12, 0, 20000)],
    }[name]
    sp = SPECIAL if name not in ("asinh", "sinh", "cosh", "tand") else np.array([0.0, 1.0, 2.0, 1e-8])
    if name in ("sin", "cos"):
        sp = sp[np.abs(sp) < 1e6]
    if name in ("sind", "cosd"):
        sp = sp[np.isfinite(sp)]
    if name in ("asin", "acos"):
        sp = sp[np.abs(sp) <= 1]
    return np.concatenate(parts + [sp])


@pytest.mark.parametrize("name", list(SCALAR))
def test_device_scalar_equals_oracle(osg, oracle, gpu, name):
    x = args_for(name, np.random.default_rng(sum(map(ord, name))))
    got, _ = probe(osg, gpu, SCALAR[name], x)
    want = oracle.math_probe(name, x)
    bad = ~same_bits(got, want)
    assert not bad.any(), (f"{name}: {bad.sum()} of {x.size} differ, e.g. x={x[bad][:3]!r} "
                           f"got={got[bad][:3]!r} want={want[bad][:3]!r}")


def _sp(pred):
    return SPECIAL[pred(SPECIAL)]


BATCH = [
    # (batch probe id, scalar probe id, argument generator, fast domain: predicate | None (everywhere) | "flag")
    (100, 0, lambda r: np.concatenate([r.uniform(-1.2, 1.2, N), r.uniform(-1e-3, 1e-3, N // 2),
                                       10.0 ** r.uniform(-320, -5, 4000), _sp(lambda s: np.abs(s) < 4)]),
     lambda x: np.abs(x) <= np.pi / 4),
    (101, 1, lambda r: np.concatenate([r.uniform(-2.3, 2.3, N), np.pi / 2 + r.uniform(-1e-4, 1e-4, 4000),
                                       np.array([0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi / 4])]), "flag"),
    (102, 5, lambda r: np.concatenate([r.uniform(-5, 5, N), 10.0 ** r.uniform(-40, 80, N // 4) * r.choice([-1, 1], N // 4),
                                       SPECIAL]), None),
    (103, 5, lambda r: np.concatenate([r.uniform(-5, 5, N), 10.0 ** r.uniform(-40, 80, N // 4) * r.choice([-1, 1], N // 4),
                                       SPECIAL]), None),
    (104, 5, lambda r: np.concatenate([r.uniform(-0.6, 0.6, N), 10.0 ** r.uniform(-40, 0, N // 4), _sp(lambda s: np.abs(s) < 2)]),
     lambda x: np.abs(x) < 0.4375),
    (105, 6, lambda r: np.concatenate([r.uniform(-0.7, 0.7, N), 10.0 ** r.uniform(-40, 0, N // 4), _sp(lambda s: np.abs(s) <= 1)]),
     lambda x: np.abs(x) < 0.5),
    (106, 2, lambda r: np.concatenate([r.uniform(-359.9, 359.9, N), np.arange(-345, 346, 15.0),
                                       np.array([0.0, -0.0, 359.99999999999994])]), None),
    (107, 3, lambda r: np.concatenate([r.uniform(-359.9, 359.9, N), np.arange(-345, 346, 15.0),
                                       np.array([0.0, -0.0, 359.99999999999994])]), None),
    # latitude-domain forms (round 3): sind / cosd for |x| <= 90, cos for |a| <= pi/2 -- flagged `rare` outside
    (108, 2, lambda r: np.concatenate([r.uniform(-95, 95, N), np.arange(-120, 121, 15.0), 45 + r.uniform(-1e-9, 1e-9, 4000),
                                       np.array([0.0, -0.0, 90.0, -90.0, 45.0, -45.0, 89.99999999999999, 5e-324, 1e-310])]),
     lambda x: np.abs(x) <= 90.0),
    (109, 3, lambda r: np.concatenate([r.uniform(-95, 95, N), np.arange(-120, 121, 15.0), 45 + r.uniform(-1e-9, 1e-9, 4000),
                                       np.array([0.0, -0.0, 90.0, -90.0, 45.0, -45.0, 89.99999999999999, 5e-324, 1e-310])]),
     lambda x: np.abs(x) <= 90.0),
    (110, 1, lambda r: np.concatenate([r.uniform(-1.7, 1.7, N), np.pi / 2 + r.uniform(-1e-4, 1e-4, 4000), np.pi / 4 + r.uniform(-1e-9, 1e-9, 4000),
                                       np.array([0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi / 4, -np.pi / 4, 2.4, -2.4, 3.2])]), "flag"),
]


@pytest.mark.parametrize("bid,sid,gen,domain", BATCH, ids=[str(b[0]) for b in BATCH])
def test_batch_form_equals_scalar(osg, gpu, bid, sid, gen, domain):
    x = gen(np.random.default_rng(bid))
    x = np.ascontiguousarray(x[: (x.size // 4) * 4])   # whole groups of 4 (the flag is per group)
    got, rare = probe(osg, gpu, bid, x)
    want, _ = probe(osg, gpu, sid, x)
    ok = same_bits(got, want)
    if domain is None:
        assert ok.all(), f"{(~ok).sum()} mismatches, e.g. x={x[~ok][:3]!r} got={got[~ok][:3]!r} want={want[~ok][:3]!r}"
        return
    if domain == "flag":                               # cos_b: wherever the group is not flagged the bits must match
        bad = ~ok & ~rare
        assert not bad.any(), f"{bad.sum()} unflagged mismatches, e.g. x={x[bad][:3]!r}"
        assert rare.mean() < (0.02 if bid == 101 else 0.12)      # cos_lat_b also flags |a| beyond a latitude (|n| > 1)
        return
    inside = domain(x)
    grp = inside.reshape(-1, 4).all(axis=1).repeat(4)  # a group is fast iff all 4 arguments are inside
    bad = inside & ~ok
    assert not bad.any(), f"{bad.sum()} mismatches inside the fast domain, e.g. x={x[bad][:3]!r} got={got[bad][:3]!r} want={want[bad][:3]!r}"
    assert np.array_equal(rare, ~grp), "rare flag must be raised exactly for groups with an outside argument"


def test_unscaled_sqrt_and_division_are_ieee_on_their_domain(osg, gpu):
    """csrc/tpg_math.hpp sqrt_nr / div_nr drop the range scaling and special-case fix-up of the compiler's
    expansions; on the operand ranges the metric kernel feeds them they must return the correctly rounded
    IEEE result (numpy's sqrt and / are correctly rounded)."""
    r = np.random.default_rng(77)
    x = np.concatenate([r.uniform(0, 2, N), 10.0 ** r.uniform(-200, 200, N), np.array([0.0, 1.0, 4.0, 2.0 ** -700, 1e-34, 1e300])])
    got, _ = probe(osg, gpu, 20, x)
    assert same_bits(got, np.sqrt(x)).all()
    got, _ = probe(osg, gpu, 20, np.array([np.nan, -1.0]))
    assert np.isnan(got).all()
    # divisions of the kernel: triangle tangents (|a| <= 2 incl. 0 and tiny, 1e-16 <= |b| <= 4), asin's p / q
    # (q in (0.7, 1]), atan's reduced argument (1 <= b <= 1.5 * 2^1000)
    a = np.concatenate([r.uniform(-2, 2, N), 10.0 ** r.uniform(-60, 0.3, N), np.zeros(1000), r.uniform(-1, 1, N), -np.ones(N // 2)])
    b = np.concatenate([r.uniform(1e-3, 4, N) * r.choice([-1, 1], N), 10.0 ** r.uniform(-16, 0.6, N), r.uniform(0.5, 4, 1000),
                        r.uniform(0.7, 1.0, N), np.concatenate([10.0 ** r.uniform(0, 300, N // 2 - 3), np.array([2.0 ** 1000, 1.5 * 2.0 ** 1000, 1.0])])])
    # ... and the Murray map's y / x (round 3): products of table entries, |x| from ~1e-17 (next to a pole meridian) to ~1e2
    a2 = 10.0 ** r.uniform(-20, 3, N) * r.choice([-1, 1], N)
    b2 = 10.0 ** r.uniform(-18, 3, N) * r.choice([-1, 1], N)
    a, b = np.concatenate([a, a2, np.zeros(100)]), np.concatenate([b, b2, 10.0 ** r.uniform(-18, 3, 100)])
    xy = np.empty(2 * a.size)
    xy[0::2], xy[1::2] = a, b
    got, _ = probe(osg, gpu, 21, xy)
    want = a / b
    assert same_bits(got[0::2], want).all() and same_bits(got[1::2], want).all()
