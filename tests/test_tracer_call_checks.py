"""The centred, the WENO5 x-y and the WENO5 x-y-z tracer tendency answer a bad call alike (no GPU): one table of fabricated calls, one per
check the three entry points have in common, goes through tpg_tracer_advection_tendency (scheme = 0), tpg_weno_tracer_advection_tendency
and tpg_weno_xyz_tracer_advection_tendency, and status and full message must be equal.  Only the halo refusal may differ, and only in the
stencil it names and the halo that stencil needs.  Every call fails in validation, none reaches a launch; the pointers are never
dereferenced."""
import ctypes as C

import pytest

GEOM = (48, 40, 3, 4, 4, 4)                                        # Nx, Ny, Nz, Hx, Hy, Hz
PLANE = 56 * 48 * 8
PARENT = PLANE * 11                                                # bytes of a Float64 parent of c, G, u, v; w has one plane more
BASE, FAR = 1 << 30, 1 << 40
SHARED = dict(u=BASE, v=BASE + PARENT, w=BASE + 2 * PARENT, dy=1 << 20, dx=2 << 20, az=3 << 20, dz=4 << 20)
TRACER = lambda q: FAR + 3 * q * PARENT                           # noqa: E731  disjoint tracers, two parents apart
TEND = lambda q: 2 * FAR + 3 * q * PARENT                          # noqa: E731  and their tendencies
HALO_FORMAT = "the rule reads {}, u[i+1, j] and v[i, j+1]: Hx >= {m}, Hy >= {m} and Hz >= 1 needed (halo ({},{},{}))"
STENCILS = {"centred": ("c[i-1..i+1, j-1..j+1, k-1..k+1]", 1), "weno": ("c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-1..k+1]", 3),
            "weno_xyz": ("c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1]", 3)}
WENO_HALO = ("the rule reads c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-1..k+1], u[i+1, j] and v[i, j+1]: "
             "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo ({},{},{}))")
WENO_XYZ_HALO = ("the rule reads c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1], u[i+1, j] and v[i, j+1]: "
                 "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo ({},{},{}))")


def _cases(n):
    """(what it is, status, message, keyword arguments of _call) per shared check, for a call of n tracers; the last tracer is the bad one"""
    q = n - 1
    aligned = "pointer not aligned to its element type"
    why = " (every item reads cells while its neighbours write)"
    tracers, tends = [TRACER(p) for p in range(n)], [TEND(p) for p in range(n)]
    put = lambda table, value: table[:q] + [value]                # noqa: E731
    cases = [("count 0", -1, "no tracers (nfields = 0)", dict(nfields=0)),
             ("count 17", -1, "17 tracers: at most TPG_MAX_FIELDS = 16 in one call", dict(nfields=17)),
             ("null c table", -1, "null table of tracers or of tendencies", dict(c=None)),
             ("null G table", -1, "null table of tracers or of tendencies", dict(G=None)),
             ("null tracer", -1, f"null tracer {q}", dict(c=put(tracers, None))),
             ("null G", -1, f"null G of tracer {q}", dict(G=put(tends, None)))]
    cases += [(f"null {name}", -1, "null u, v or w", dict(shared={name: None})) for name in ("u", "v", "w")]
    cases += [(f"null {name}", -1, "null dy_fc, dx_cf, az_cc or dz_c", dict(shared={name: None})) for name in ("dy", "dx", "az", "dz")]
    cases += [("misaligned tracer", -1, f"tracer {q}: {aligned}", dict(c=put(tracers, TRACER(q) + 4))),
              ("misaligned G", -1, f"G of tracer {q}: {aligned}", dict(G=put(tends, TEND(q) + 4)))]
    cases += [(f"misaligned {name}", -1, f"u, v or w {aligned}", dict(shared={name: SHARED[name] + 4})) for name in ("u", "v", "w")]
    cases += [(f"misaligned {name}", -1, f"dy_fc, dx_cf, az_cc or dz_c {aligned}", dict(shared={name: SHARED[name] + 4}))
              for name in ("dy", "dx", "az", "dz")]
    cases += [("misaligned count plane", -1, "count plane pointer not aligned to int32", dict(n_cc=(5 << 20) + 2)),
              ("G on a tracer", -1, f"G of tracer {q} overlaps tracer 0{why}", dict(G=put(tends, TRACER(0) + 8)))]
    cases += [(f"G on {name}", -1, f"G of tracer {q} overlaps {name}{why}", dict(G=put(tends, SHARED[name] + PARENT - 8))) for name in ("u", "v", "w")]
    if n > 1:
        cases.append(("G on a G", -1, f"G of tracer {q} overlaps G of tracer 0", dict(G=put(tends, TEND(0) - 8))))
    return cases


def _call(kind, lib, n, nfields=None, shared=None, n_cc=None, geom=GEOM, **tables):
    c = tables.get("c", [TRACER(p) for p in range(n)])
    G = tables.get("G", [TEND(p) for p in range(n)])
    c, G = (t if t is None else (C.c_void_p * len(t))(*t) for t in (c, G))
    s = {**SHARED, **(shared or {})}
    head = (c, G, n if nfields is None else nfields, s["u"], s["v"], s["w"], s["dy"], s["dx"], s["az"], s["dz"], n_cc, 0.0)
    if kind == "centred":
        return lib.tpg_tracer_advection_tendency(*head, 0, *geom, 1, None), lib.tpg_advection_last_error().decode()
    if kind == "weno_xyz":
        return lib.tpg_weno_xyz_tracer_advection_tendency(*head, *geom, 1, None), lib.tpg_weno_xyz_last_error().decode()
    return lib.tpg_weno_tracer_advection_tendency(*head, *geom, 1, None), lib.tpg_weno_last_error().decode()


@pytest.fixture(scope="module")
def libs(osg):
    return {"centred": osg._lib.advection_lib(), "weno": osg._lib.weno_lib(), "weno_xyz": osg._lib.weno_xyz_lib()}


@pytest.mark.parametrize("n", [1, 2, 16])
def test_shared_checks_answer_alike(libs, n):
    for what, status, message, kw in _cases(n):
        got = {kind: _call(kind, lib, n, **kw) for kind, lib in libs.items()}
        assert got["centred"] == got["weno"] == got["weno_xyz"] == (status, message), (what, n)


@pytest.mark.parametrize("n", [1, 2, 16])
@pytest.mark.parametrize("halo", [(4, 4, 0), (0, 0, 0)])
def test_halo_refusals_differ_in_the_stencil_only(libs, n, halo):
    assert set(libs) == set(STENCILS)
    for kind, lib in libs.items():
        stencil, least = STENCILS[kind]
        assert _call(kind, lib, n, geom=GEOM[:3] + halo) == (-5, HALO_FORMAT.format(stencil, *halo, m=least)), (kind, n)
    # a halo the centred stencil has room in, and the two WENO sentences written out: one sentence around the stencil and its minimum
    assert _call("weno", libs["weno"], n, geom=GEOM[:3] + (2, 4, 4)) == (-5, WENO_HALO.format(2, 4, 4))
    assert _call("weno_xyz", libs["weno_xyz"], n, geom=GEOM[:3] + (2, 4, 4)) == (-5, WENO_XYZ_HALO.format(2, 4, 4))
    for kind, literal in (("weno", WENO_HALO), ("weno_xyz", WENO_XYZ_HALO)):
        stencil, least = STENCILS[kind]
        assert HALO_FORMAT.format(stencil, *halo, m=least) == literal.format(*halo)
