"""Host-side tests of the tracer tendency of `WENO()` (no GPU): the export list of libtripolar_hip_weno_xyz.so, every argument error of
tpg_weno_xyz_tracer_advection_tendency in the header's order (status and message; every call below fails in validation, none reaches a
launch, the pointers are fabricated and never dereferenced) -- from ONE table of bad calls that goes through
tpg_weno_tracer_advection_tendency too, where status and message must be equal --, every refusal and every accepted scheme of the Python
layer on host-only grid records, the loader, and that the Makefile and the argument-check tool name the library."""
import ctypes as C
import os

import pytest

NAMES = ["tpg_weno_xyz_last_error", "tpg_weno_xyz_tracer_advection_tendency"]
GEOM = (48, 40, 3, 4, 4, 4)                                        # Nx, Ny, Nz, Hx, Hy, Hz
PLANE = 56 * 48 * 8
PARENT, WPARENT = PLANE * 11, PLANE * 12                           # bytes of a Float64 parent of c, G, u, v (Nz + 2Hz planes) and of w (one more)
BASE, FAR = 1 << 30, 1 << 40
SHARED = dict(u=BASE, v=BASE + PARENT, w=BASE + 2 * PARENT, dy=1 << 20, dx=2 << 20, az=3 << 20, dz=4 << 20)
N_CC = 5 << 20
TRACER = lambda q: FAR + 3 * q * PARENT                           # noqa: E731  disjoint tracers, two parents apart
TEND = lambda q: 2 * FAR + 3 * q * PARENT                          # noqa: E731  and their tendencies
HALO_FORMAT = "the rule reads {}, u[i+1, j] and v[i, j+1]: Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo ({},{},{}))"
STENCILS = {"weno": "c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-1..k+1]",
            "weno_xyz": "c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1]"}
WHY = " (every item reads cells while its neighbours write)"
ALIGNED = "pointer not aligned to its element type"


def _bad_calls(n):
    """(what it is, status, message, keyword arguments of _call), in the order of the header's list of refusals, for a call of n tracers of
    which the last is the bad one.  A message of None: whatever the library says (the status alone is the header's)."""
    q = n - 1
    tracers, tends = [TRACER(p) for p in range(n)], [TEND(p) for p in range(n)]
    put = lambda table, value: table[:q] + [value]                # noqa: E731
    rows = [  # 1. the geometry
        ("unknown ft", -1, "unknown element type ft=7", dict(ft=7)),
        ("odd Nx", -2, None, dict(geom=(49, 40, 3, 4, 4, 4))),
        ("Nz = 0", -1, None, dict(geom=(48, 40, 0, 4, 4, 4))),
        ("Hz < 0", -1, None, dict(geom=(48, 40, 3, 4, 4, -1))),
        # 2. the number of tracers
        ("count 0", -1, "no tracers (nfields = 0)", dict(nfields=0)),
        ("count -3", -1, "no tracers (nfields = -3)", dict(nfields=-3)),
        ("count 17", -1, "17 tracers: at most TPG_MAX_FIELDS = 16 in one call", dict(nfields=17)),
        # 3. the tables and their entries
        ("null c table", -1, "null table of tracers or of tendencies", dict(c=None)),
        ("null G table", -1, "null table of tracers or of tendencies", dict(G=None)),
        ("null tracer", -1, f"null tracer {q}", dict(c=put(tracers, None))),
        ("null G", -1, f"null G of tracer {q}", dict(G=put(tends, None)))]
    # 4. the velocities and the metrics
    rows += [(f"null {name}", -1, "null u, v or w", dict(shared={name: None})) for name in ("u", "v", "w")]
    rows += [(f"null {name}", -1, "null dy_fc, dx_cf, az_cc or dz_c", dict(shared={name: None})) for name in ("dy", "dx", "az", "dz")]
    # 5. alignment, Float64 and Float32
    rows += [("misaligned tracer", -1, f"tracer {q}: {ALIGNED}", dict(c=put(tracers, TRACER(q) + 4))),
             ("misaligned tracer, Float32", -1, f"tracer {q}: {ALIGNED}", dict(c=put(tracers, TRACER(q) + 2), ft=0)),
             ("misaligned G", -1, f"G of tracer {q}: {ALIGNED}", dict(G=put(tends, TEND(q) + 4)))]
    rows += [(f"misaligned {name}", -1, f"u, v or w {ALIGNED}", dict(shared={name: SHARED[name] + 4})) for name in ("u", "v", "w")]
    rows += [(f"misaligned {name}", -1, f"dy_fc, dx_cf, az_cc or dz_c {ALIGNED}", dict(shared={name: SHARED[name] + 4})) for name in ("dy", "dx", "az", "dz")]
    rows += [(f"misaligned {name}, Float32", -1, f"dy_fc, dx_cf, az_cc or dz_c {ALIGNED}", dict(shared={name: SHARED[name] + 2}, ft=0))
             for name in ("dy", "dx", "az", "dz")]
    rows += [("misaligned count plane", -1, "count plane pointer not aligned to int32", dict(n_cc=N_CC + 2))]
    # 6. the overlaps: identical, one element inside from either side
    for shift in (0, 8, -8, PARENT - 8, 8 - PARENT):
        rows.append((f"G on a tracer {shift:+d}", -1, f"G of tracer {q} overlaps tracer 0{WHY}", dict(G=put(tends, TRACER(0) + shift))))
        rows += [(f"G on {name} {shift:+d}", -1, f"G of tracer {q} overlaps {name}{WHY}",
                  dict(G=put(tends, SHARED[name] + shift), shared={o: (3 + i) * FAR for i, o in enumerate("uvw") if o != name})) for name in ("u", "v")]
        if n > 1:
            rows.append((f"G on a G {shift:+d}", -1, f"G of tracer {q} overlaps G of tracer 0", dict(G=put(tends, TEND(0) + shift))))
    rows += [(f"G on w {shift:+d}", -1, f"G of tracer {q} overlaps w{WHY}", dict(G=put(tends, SHARED["w"] + shift), shared=dict(u=3 * FAR, v=4 * FAR)))
             for shift in (0, 8, -8, WPARENT - 8, 8 - PARENT)]     # w's parent is one level longer
    return rows


def _call(kind, lib, n, nfields=None, shared=None, n_cc=None, geom=GEOM, ft=1, **tables):
    c = tables.get("c", [TRACER(p) for p in range(n)])
    G = tables.get("G", [TEND(p) for p in range(n)])
    c, G = (t if t is None else (C.c_void_p * len(t))(*t) for t in (c, G))
    s = {**SHARED, **(shared or {})}
    args = (c, G, n if nfields is None else nfields, s["u"], s["v"], s["w"], s["dy"], s["dx"], s["az"], s["dz"], n_cc, 0.0, *geom, ft, None)
    if kind == "weno":
        return lib.tpg_weno_tracer_advection_tendency(*args), lib.tpg_weno_last_error().decode()
    return lib.tpg_weno_xyz_tracer_advection_tendency(*args), lib.tpg_weno_xyz_last_error().decode()


@pytest.fixture(scope="module")
def libs(osg):
    return {"weno": osg._lib.weno_lib(), "weno_xyz": osg._lib.weno_xyz_lib()}


def test_header_map_and_library_export_exactly_the_two_names(osg):
    from test_abi import ROOT, declared_symbols, exported_symbols
    osg._lib.weno_xyz_lib()
    assert declared_symbols("tripolar_hip_weno_xyz.h") == NAMES == exported_symbols(osg._lib.WENO_XYZ_LIB_PATH) == sorted(osg._lib.WENO_XYZ_SIGNATURES)
    vs = open(os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc", "weno_xyz.map")).read()
    assert all(n in vs for n in NAMES) and "local: *;" in vs and vs.count("tpg_") == 2


@pytest.mark.parametrize("n", [1, 2, 16])
def test_argument_errors_in_the_headers_order_and_as_the_existing_call_answers(libs, n):
    """every row of the one table through both calls: the status is the header's, the message the table's, and the two libraries answer
    with equal status and equal message"""
    for what, status, message, kw in _bad_calls(n):
        got = {kind: _call(kind, lib, n, **kw) for kind, lib in libs.items()}
        assert got["weno_xyz"][0] == status, (what, n, got)
        assert message is None or got["weno_xyz"][1] == message, (what, n, got)
        assert got["weno_xyz"] == got["weno"], (what, n)
    assert _call("weno_xyz", libs["weno_xyz"], 16, shared=dict(u=None)) == (-1, "null u, v or w")      # 16 tracers are accepted


def test_order_of_the_refusals(libs):
    """a call bad in two ways is refused for the earlier item of the header's list"""
    lib = libs["weno_xyz"]
    two = lambda **kw: _call("weno_xyz", lib, 2, **kw)            # noqa: E731
    assert two(ft=7, nfields=0)[1] == "unknown element type ft=7"                                         # 1 before 2
    assert two(nfields=0, c=None)[1] == "no tracers (nfields = 0)"                                        # 2 before 3
    assert two(c=None, shared=dict(u=None))[1] == "null table of tracers or of tendencies"                # 3 before 4
    assert two(shared=dict(u=None, dy=SHARED["dy"] + 4))[1] == "null u, v or w"                           # 4 before 5
    assert two(shared=dict(u=None, dz=None))[1] == "null u, v or w"                                       # 4: the velocities first
    assert two(n_cc=N_CC + 2, G=[TEND(0), TRACER(0)])[1] == "count plane pointer not aligned to int32"     # 5 before 6
    assert two(G=[TEND(0), TRACER(0)], geom=(48, 40, 3, 4, 4, 0))[1].startswith("G of tracer 1 overlaps tracer 0")   # 6 before 7
    # exact: G right behind or right in front of an array is no overlap (the call goes on to refuse Hz = 0), one element nearer is
    h0, p0 = (48, 40, 3, 4, 4, 0), PLANE * 3
    for shift, status in ((p0, -5), (p0 - 8, -1), (-p0, -5), (8 - p0, -1)):
        assert two(G=[TEND(0), TRACER(0) + shift], geom=h0)[0] == status, shift
    # 8. more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    big = dict(c=[1 << 44], G=[2 << 44], shared=dict(u=5 << 44, v=6 << 44, w=7 << 44), ft=0)
    status, message = _call("weno_xyz", lib, 1, geom=(65536, 32768, 1, 3, 3, 1), **big)
    assert status == -5 and "32-bit" in message


@pytest.mark.parametrize("n", [1, 16])
def test_halo_refusal_names_this_calls_stencil(libs, n):
    """7. Hx < 3, Hy < 3 or Hz < 1, one direction at a time and all at once, both types: the message differs from the existing call's in the
    stencil only"""
    for halo in ((2, 4, 4), (4, 2, 4), (4, 4, 0), (0, 4, 4), (4, 1, 4), (0, 0, 0)):
        for ft in (0, 1):
            for kind, lib in libs.items():
                assert _call(kind, lib, n, geom=GEOM[:3] + halo, ft=ft, n_cc=N_CC) == (-5, HALO_FORMAT.format(STENCILS[kind], *halo)), (kind, halo)
    for halo in ((3, 3, 1), (3, 4, 4)):                            # the narrowest halo accepted: the call goes on (to the launch it must not reach here)
        assert _call("weno_xyz", libs["weno_xyz"], n, geom=GEOM[:3] + halo, shared=dict(u=None)) == (-1, "null u, v or w")


def _grid(osg, Hx=3, Hy=3, Hz=1, **kw):
    """an OrthogonalSphericalShellGrid record with host tensors: enough for the checks that touch no device"""
    import torch
    Nz = 3
    a = dict(architecture=None, Nx=8, Ny=6, Nz=Nz, Hx=Hx, Hy=Hy, Hz=Hz, Lz=1.0,
             arrays={"lambda_cc": torch.zeros(6 + 2 * Hy, 8 + 2 * Hx, dtype=torch.float64)},
             z_faces=torch.zeros(Nz + 1 + 2 * Hz), z_centers=torch.zeros(Nz + 2 * Hz), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
             topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=torch.float64, z_spec=(-1, 0))
    a.update(kw)
    return osg.OrthogonalSphericalShellGrid(**a)


def test_python_refusals_and_accepted_schemes(osg, monkeypatch):
    import torch
    for name in ("weno_xyz_tracer_advection_tendency", "weno_xyz_tracer_advection_plan", "WenoXyzTracerAdvectionPlan"):
        assert hasattr(osg, name), name
    for name in ("weno_xyz_lib", "check_weno_xyz", "WENO_XYZ_SIGNATURES", "WENO_XYZ_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    Plan = osg.WenoXyzTracerAdvectionPlan
    assert issubclass(Plan, osg._operator_plan.OperatorPlan) and issubclass(Plan, osg.advection._TracerTendencyPlan)
    assert Plan._HALO == (3, 3, 1) and Plan._LIBRARY == ("weno_xyz_lib", "check_weno_xyz", "tpg_weno_xyz_tracer_advection_tendency")
    grid, other = _grid(osg), _grid(osg)
    new_c = lambda g=grid, **kw: osg.CenterField(g, **kw)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, d, Gc, Gd = new_c(), new_c(), new_c(), new_c()
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))
    window = (slice(None), slice(None), range(1, 3))
    FF, WENO, Centered = osg.FluxFormAdvection, osg.WENO, osg.Centered
    # the accepted schemes, all the same thing: the plan's construction gets past the scheme (and every other check of these host records)
    # to the library's loader, which is made to say so
    reached = []
    monkeypatch.setattr(osg._lib, "weno_xyz_lib", lambda: reached.append(1) or (_ for _ in ()).throw(RuntimeError("reached the loader")))
    for kw in (dict(), dict(scheme=WENO()), dict(scheme=WENO(order=5)), dict(scheme=FF(WENO(), WENO(), WENO())),
               dict(scheme=FF(WENO(order=5), WENO(), WENO(order=5)))):
        with pytest.raises(RuntimeError, match="reached the loader"):
            osg.weno_xyz_tracer_advection_plan([c], u, v, w, [Gc], **kw)
        with pytest.raises(RuntimeError, match="reached the loader"):
            osg.weno_xyz_tracer_advection_tendency([c], u, v, w, out=[Gc], **kw)
    assert len(reached) == 10
    for fn in (osg.weno_xyz_tracer_advection_plan, lambda t, u_, v_, w_, G, **kw: osg.weno_xyz_tracer_advection_tendency(t, u_, v_, w_, out=G, **kw)):
        with pytest.raises(TypeError, match="no tracers"):
            fn([], u, v, w, [])
        with pytest.raises(TypeError, match=r"lists of one length \(2, 1\)"):
            fn([c, d], u, v, w, [Gc])
        # the scheme: everything else is refused, and the message names what is built
        built = r"is not built.* \(WENO\(order=5\), the same as FluxFormAdvection\(WENO\(order=5\), WENO\(order=5\), WENO\(order=5\)\) is"
        for scheme in (WENO(order=7), WENO(order=3), FF(WENO(), WENO(), Centered()), FF(WENO(), WENO(), WENO(order=7)), FF(WENO(order=3), WENO(), WENO()),
                       FF(Centered(), Centered(), Centered()), FF(WENO(), Centered(), WENO()), "weno5", "WENO()", None, Centered(), 5):
            with pytest.raises(NotImplementedError, match=built):
                fn([c], u, v, w, [Gc], scheme=scheme)
        with pytest.raises(NotImplementedError, match=r"is not built \(weno_tracer_advection_tendency has it\)"):
            fn([c], u, v, w, [Gc], scheme=osg.weno.BUILT)
        with pytest.raises(NotImplementedError) as err:
            fn([c], u, v, w, [Gc], scheme=WENO(order=7))
        assert "weno_tracer_advection_tendency has it" not in str(err.value)
        # locations
        with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
            fn([c], v, v, w, [Gc])
        with pytest.raises(TypeError, match=r"v must be a Field at \(Center, Face, Center\)"):
            fn([c], u, c, w, [Gc])
        with pytest.raises(TypeError, match=r"w must be a Field at \(Center, Center, Face\)"):
            fn([c], u, v, c, [Gc])
        with pytest.raises(TypeError, match=r"tracer 1 must be a Field at \(Center, Center, Center\)"):
            fn([c, osg.XFaceField(grid)], u, v, w, [Gc, Gd])
        with pytest.raises(TypeError, match=r"G of tracer 1 must be a Field at \(Center, Center, Center\)"):
            fn([c, d], u, v, w, [Gc, osg.ZFaceField(grid)])
        # one grid, one type, no z-window
        with pytest.raises(ValueError, match="one grid"):
            fn([c, new_c(other)], u, v, w, [Gc, Gd])
        with pytest.raises(ValueError, match="one element type"):
            fn([c, d], u, v, f32(osg.ZFaceField), [Gc, Gd])
        with pytest.raises(NotImplementedError, match="z-windowed"):
            fn([c, new_c(indices=window)], u, v, w, [Gc, Gd])
        # aliases, by identity
        with pytest.raises(ValueError, match="G of tracer 0 is tracer 0 itself"):
            fn([c], u, v, w, [c])
        with pytest.raises(ValueError, match="G of tracer 1 and G of tracer 0 are one field"):
            fn([c, d], u, v, w, [Gc, Gc])
        # a halo narrower than (3, 3, 1), one direction at a time: this plan's own sentence
        for halo in ((2, 3, 1), (3, 2, 1), (3, 3, 0), (1, 1, 1)):
            thin = _grid(osg, *halo)
            with pytest.raises(ValueError, match=rf"the planes 0 and Nz \+ 1 only.*the halo must be at least \(3, 3, 1\) \(halo \({halo[0]}, {halo[1]}, {halo[2]}\)\)"):
                fn([new_c(thin)], osg.XFaceField(thin), osg.YFaceField(thin), osg.ZFaceField(thin), [new_c(thin)])
        # a latitude band
        band = _grid(osg, topology=(osg.PeriodicTopology, osg.FullyConnected, osg.Bounded), global_size=(8, 12, 3), jrange=(1, 6))
        with pytest.raises(NotImplementedError, match="latitude-band grids are not handled: the rows Ny \\+ 1 .. Ny \\+ 3 of a band are exchanged"):
            fn([new_c(band)], osg.XFaceField(band), osg.YFaceField(band), osg.ZFaceField(band), [new_c(band)])
    # out=None allocates only after the tracers are known to be Center fields
    with pytest.raises(TypeError, match=r"tracer 0 must be a Field at \(Center, Center, Center\)"):
        osg.weno_xyz_tracer_advection_tendency([u], u, v, w)
    # the existing call keeps refusing the all-WENO schemes, and now says where they are
    for scheme in (WENO(), FF(WENO(), WENO(), WENO())):
        with pytest.raises(NotImplementedError, match=r"is not built \(FluxFormAdvection\(WENO\(order=5\), WENO\(order=5\), Centered\(\)\) is.*weno_xyz_tracer_advection_tendency"):
            osg.weno_tracer_advection_plan([c], u, v, w, [Gc], scheme=scheme)


def test_build_and_documents_name_the_library():
    """the Makefile keeps contraction off, the face value
    of order three sits beside weno_face, and the argument-check program is a stand-alone one with the sanitizer build line in its header"""
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "-ffp-contract=off" in mk
    tool = open(os.path.join(ROOT, "tools", "tracer_argcheck.cpp")).read()                    # one program over the three tracer calls
    assert "int main()" in tool and "-Xarch_host -fsanitize=address,undefined" in tool and "tpg_weno_xyz.hip" in tool
    assert "tpg_weno_xyz_tracer_advection_tendency" in tool and "csrc/tpg_advection.hip" in tool and "csrc/tpg_weno.hip" in tool
    # the library's file and the kernel header it includes, together
    hip = open(os.path.join(csrc, "tpg_weno_xyz.hip")).read()
    assert '#include "tpg_weno_tracer_kernel.hpp"' in hip and "__global__" not in hip
    assert "TPG_WXYZ" not in open(os.path.join(csrc, "tpg_weno_tracer_kernel.hpp")).read() and "TPG_WENO_" not in hip
    src = hip + open(os.path.join(csrc, "tpg_weno_tracer_kernel.hpp")).read()
    assert '#include "tpg_tracer_tendency.hpp"' in src and '#include "tpg_weno_face.hpp"' in src and "TracerCall" in src and "check_geom" in src
    assert "weno_face3" in src and "__shared__" not in src and "atomic" not in src.replace("No atomics", "")
    face = open(os.path.join(csrc, "tpg_weno_face.hpp")).read()
    assert "T weno_face3(T q0, T q1, T q2)" in face and "T weno_face(T q0, T q1, T q2, T q3, T q4)" in face
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):
        assert "weno_xyz" in open(os.path.join(ROOT, doc)).read(), doc
