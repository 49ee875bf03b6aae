"""Host-side tests of the WENO5 tracer advection tendency (no GPU): the export list of libtripolar_hip_weno.so, every argument error of
tpg_weno_tracer_advection_tendency (status and message; every call below fails in validation, none reaches a launch, the pointers are
fabricated and never dereferenced), every refusal of the Python layer on host-only grid records, and the loader."""
import ctypes as C
import os

import pytest

NAMES = ["tpg_weno_last_error", "tpg_weno_tracer_advection_tendency"]
G = (48, 40, 3, 4, 4, 4)                                           # Nx, Ny, Nz, Hx, Hy, Hz
PLANE = 56 * 48 * 8
PARENT, WPARENT = PLANE * 11, PLANE * 12                           # bytes of a Float64 parent of c, G, u, v (Nz + 2Hz planes) and of w (one more)
BASE, FAR = 1 << 30, 1 << 40
U, V, W = BASE, BASE + PARENT, BASE + 2 * PARENT
DY, DX, AZ, DZ, N = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20
TRACER = lambda q: FAR + 3 * q * PARENT                           # noqa: E731  disjoint tracers, two parents apart
TEND = lambda q: 2 * FAR + 3 * q * PARENT                          # noqa: E731  and their tendencies


def _table(addresses):
    return (C.c_void_p * len(addresses))(*addresses)


def _call(lib, c=None, g=None, n=2, shared=None, n_cc=None, geom=G, ft=1, tables=True):
    c = [TRACER(q) for q in range(max(n, 1))] if c is None else c
    g = [TEND(q) for q in range(max(n, 1))] if g is None else g
    s = dict(u=U, v=V, w=W, dy=DY, dx=DX, az=AZ, dz=DZ)
    s.update(shared or {})
    ct, gt = (_table(c), _table(g)) if tables is True else tables
    return lib.tpg_weno_tracer_advection_tendency(ct, gt, n, s["u"], s["v"], s["w"], s["dy"], s["dx"], s["az"], s["dz"], n_cc, 0.0, *geom, ft, None)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import ROOT, declared_symbols, exported_symbols
    osg._lib.weno_lib()
    assert declared_symbols("tripolar_hip_weno.h") == NAMES == exported_symbols(osg._lib.WENO_LIB_PATH) == sorted(osg._lib.WENO_SIGNATURES)
    # the centred call keeps refusing every scheme but its own: the feature is this library, not a new value of that argument
    assert osg._lib.TPG_ADVECTION_CENTERED2 == 0 and not hasattr(osg._lib, "TPG_ADVECTION_WENO5")


def test_argument_errors_without_device_work(osg):
    lib = osg._lib.weno_lib()
    err = lambda: lib.tpg_weno_last_error().decode()
    # 1. the geometry
    assert _call(lib, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _call(lib, geom=(49, 40, 3, 4, 4, 4)) == -2
    assert _call(lib, geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert _call(lib, geom=(48, 40, 3, 4, 4, -1)) == -1 and err().startswith("invalid size")
    # 2. the number of tracers
    assert _call(lib, n=0) == -1 and err() == "no tracers (nfields = 0)"
    assert _call(lib, n=-3) == -1 and err() == "no tracers (nfields = -3)"
    assert _call(lib, n=17) == -1 and err() == "17 tracers: at most TPG_MAX_FIELDS = 16 in one call"
    assert _call(lib, n=16, shared=dict(u=None)) == -1 and err() == "null u, v or w"     # 16 are accepted
    # 3. the tables and their entries
    assert _call(lib, tables=(None, _table([TEND(0), TEND(1)]))) == -1 and err() == "null table of tracers or of tendencies"
    assert _call(lib, tables=(_table([TRACER(0), TRACER(1)]), None)) == -1 and err() == "null table of tracers or of tendencies"
    assert _call(lib, c=[TRACER(0), None, TRACER(2)], n=3) == -1 and err() == "null tracer 1"
    assert _call(lib, g=[TEND(0), TEND(1), None], n=3) == -1 and err() == "null G of tracer 2"
    # 4. the velocities and the metrics
    for name in ("u", "v", "w"):
        assert _call(lib, shared={name: None}) == -1 and err() == "null u, v or w"
    for name in ("dy", "dx", "az", "dz"):
        assert _call(lib, shared={name: None}) == -1 and err() == "null dy_fc, dx_cf, az_cc or dz_c"
    # 5. alignment: to the element type, Float64 and Float32, and the count plane to int32
    assert _call(lib, c=[TRACER(0), TRACER(1) + 4]) == -1 and err() == "tracer 1: pointer not aligned to its element type"
    assert _call(lib, c=[TRACER(0), TRACER(1) + 2], ft=0) == -1 and err() == "tracer 1: pointer not aligned to its element type"
    assert _call(lib, g=[TEND(0) + 4, TEND(1)]) == -1 and err() == "G of tracer 0: pointer not aligned to its element type"
    for name in ("u", "v", "w"):
        assert _call(lib, shared={name: BASE + 3 * PARENT + 4}) == -1 and err() == "u, v or w pointer not aligned to its element type"
    for name, at in (("dy", DY), ("dx", DX), ("az", AZ), ("dz", DZ)):
        assert _call(lib, shared={name: at + 4}) == -1 and err() == "dy_fc, dx_cf, az_cc or dz_c pointer not aligned to its element type"
        assert _call(lib, shared={name: at + 2}, ft=0) == -1 and err() == "dy_fc, dx_cf, az_cc or dz_c pointer not aligned to its element type"
    assert _call(lib, n_cc=N + 2) == -1 and err() == "count plane pointer not aligned to int32"
    # 6. the overlaps: any G against any tracer, u, v, w and another G -- identical, one element inside from either side
    for shift in (0, 8, -8, PARENT - 8, 8 - PARENT):
        assert _call(lib, g=[TEND(0), TRACER(0) + shift]) == -1 and err().startswith("G of tracer 1 overlaps tracer 0"), shift
        assert _call(lib, g=[TRACER(1) + shift, TEND(1)]) == -1 and err().startswith("G of tracer 0 overlaps tracer 1"), shift
        assert _call(lib, g=[TEND(0), U + shift], shared=dict(v=3 * FAR, w=4 * FAR)) == -1 and err().startswith("G of tracer 1 overlaps u"), shift
        assert _call(lib, g=[V + shift, TEND(1)], shared=dict(u=3 * FAR, w=4 * FAR)) == -1 and err().startswith("G of tracer 0 overlaps v"), shift
        assert _call(lib, g=[TEND(0), TEND(0) + shift]) == -1 and err() == "G of tracer 1 overlaps G of tracer 0", shift
    for shift in (0, 8, -8, WPARENT - 8, 8 - PARENT):              # w's parent is one level longer
        assert _call(lib, g=[TEND(0), W + shift], shared=dict(u=3 * FAR, v=4 * FAR)) == -1 and err().startswith("G of tracer 1 overlaps w"), shift
    # exact: G right behind or right in front of an array is no overlap (the call goes on to refuse Hz = 0), one element nearer is
    h0 = (48, 40, 3, 4, 4, 0)
    p0, w0 = PLANE * 3, PLANE * 4
    lone = dict(u=3 * FAR, v=4 * FAR, w=5 * FAR)
    for shift, status in ((p0, -5), (p0 - 8, -1), (-p0, -5), (8 - p0, -1)):
        assert _call(lib, g=[TEND(0), TRACER(0) + shift], geom=h0) == status, shift
        assert err().startswith("G of tracer 1 overlaps tracer 0" if status == -1 else "the rule reads")
        assert _call(lib, g=[TEND(0), TEND(0) + shift], geom=h0) == status, shift
    for shift, status in ((w0, -5), (w0 - 8, -1), (-p0, -5), (8 - p0, -1)):
        assert _call(lib, g=[TEND(0), lone["w"] + shift], shared=lone, geom=h0) == status, shift
    # the tracers, u, v and w are only read: they may be one array
    assert _call(lib, c=[TRACER(0), TRACER(0)], shared=dict(u=TRACER(0), v=TRACER(0)), geom=h0) == -5
    # 7. the halo the stencil needs, one direction at a time, both types: Hx = 2, Hy = 2, Hz = 0 (and narrower)
    for geom in ((48, 40, 3, 2, 4, 4), (48, 40, 3, 4, 2, 4), (48, 40, 3, 4, 4, 0), (48, 40, 3, 0, 4, 4), (48, 40, 3, 4, 1, 4)):
        for ft in (0, 1):
            assert _call(lib, geom=geom, ft=ft, n_cc=N) == -5, geom
            assert "c[i-3..i+3, j, k], c[i, j-3..j+3, k]" in err() and "Hx >= 3, Hy >= 3 and Hz >= 1 needed" in err()
            assert "(halo " + str(geom[3:]).replace(" ", "") + ")" in err()
    for geom in ((48, 40, 3, 3, 3, 1), (48, 40, 3, 3, 4, 4)):      # the narrowest halo accepted: the call goes on (to the launch it must not reach here)
        assert _call(lib, geom=geom, shared=dict(u=None)) == -1 and err() == "null u, v or w"
    # 8. more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    big = [1 << 44, 2 << 44]
    assert _call(lib, c=big, g=[3 << 44, 4 << 44], shared=dict(u=5 << 44, v=6 << 44, w=7 << 44), geom=(65536, 32768, 1, 3, 3, 1), ft=0) == -5
    assert "32-bit" in err()


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


def test_scheme_records(osg):
    assert osg.WENO() == osg.WENO(order=5) and osg.WENO().order == 5 and osg.WENO(order=7) != osg.WENO()
    assert osg.Centered() == osg.Centered(order=2) and osg.Centered().order == 2
    s = osg.FluxFormAdvection(osg.WENO(order=5), osg.WENO(order=5), osg.Centered())
    assert (s.x, s.y, s.z) == (osg.WENO(), osg.WENO(), osg.Centered()) and s == osg.weno.BUILT
    assert "WENO(order=5)" in repr(s) and "Centered(order=2)" in repr(s)


def test_python_refusals(osg):
    import torch
    for name in ("weno_tracer_advection_tendency", "weno_tracer_advection_plan", "WenoTracerAdvectionPlan", "WENO", "Centered", "FluxFormAdvection"):
        assert hasattr(osg, name), name
    for name in ("weno_lib", "check_weno", "WENO_SIGNATURES", "WENO_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    assert issubclass(osg.WenoTracerAdvectionPlan, osg._operator_plan.OperatorPlan)
    grid, other = _grid(osg), _grid(osg)
    new_c = lambda g=grid, **kw: osg.CenterField(g, **kw)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, d, Gc, Gd = new_c(), new_c(), new_c(), new_c()
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))
    window = (slice(None), slice(None), range(1, 3))
    FF, WENO, Centered = osg.FluxFormAdvection, osg.WENO, osg.Centered
    for fn in (osg.weno_tracer_advection_plan, lambda t, u_, v_, w_, G, **kw: osg.weno_tracer_advection_tendency(t, u_, v_, w_, out=G, **kw)):
        with pytest.raises(TypeError, match="no tracers"):
            fn([], u, v, w, [])
        with pytest.raises(TypeError, match=r"lists of one length \(2, 1\)"):
            fn([c, d], u, v, w, [Gc])
        # the scheme: exactly FluxFormAdvection(WENO(order=5), WENO(order=5), Centered()); the message names what is built
        built = r"is not built \(FluxFormAdvection\(WENO\(order=5\), WENO\(order=5\), Centered\(\)\) is"
        for scheme in (WENO(), FF(WENO(), WENO(), WENO()), FF(WENO(), WENO(), Centered(order=4)), FF(WENO(order=7), WENO(), Centered()),
                       FF(WENO(), WENO(order=3), Centered()), FF(Centered(), Centered(), Centered()), FF(WENO(), Centered(), Centered()),
                       "weno5", "centered2", None, Centered()):
            with pytest.raises(NotImplementedError, match=built):
                fn([c], u, v, w, [Gc], scheme=scheme)
        # locations
        with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
            fn([c], v, v, w, [Gc])
        with pytest.raises(TypeError, match=r"v must be a Field at \(Center, Face, Center\)"):
            fn([c], u, c, w, [Gc])
        with pytest.raises(TypeError, match=r"w must be a Field at \(Center, Center, Face\)"):
            fn([c], u, v, c, [Gc])
        with pytest.raises(TypeError, match="w must be a Field"):
            fn([c], u, v, w.data, [Gc])
        with pytest.raises(TypeError, match=r"tracer 1 must be a Field at \(Center, Center, Center\)"):
            fn([c, osg.XFaceField(grid)], u, v, w, [Gc, Gd])
        with pytest.raises(TypeError, match=r"G of tracer 1 must be a Field at \(Center, Center, Center\)"):
            fn([c, d], u, v, w, [Gc, osg.ZFaceField(grid)])
        with pytest.raises(TypeError, match="G of tracer 0 must be a Field"):
            fn([c], u, v, w, [Gc.data])
        with pytest.raises(TypeError, match="tracer 0 must be a Field at"):
            fn([osg.Field((osg.Center, osg.Center, None), grid)], u, v, w, [Gc])
        # one grid, one type, no z-window: for every field of the call
        for kw in (dict(u_=osg.XFaceField(other)), dict(v_=osg.YFaceField(other)), dict(w_=osg.ZFaceField(other)), dict(t=[c, new_c(other)]),
                   dict(G=[Gc, new_c(other)])):
            a = dict(t=[c, d], u_=u, v_=v, w_=w, G=[Gc, Gd])
            a.update(kw)
            with pytest.raises(ValueError, match="one grid"):
                fn(a["t"], a["u_"], a["v_"], a["w_"], a["G"])
        for kw in (dict(u_=f32(osg.XFaceField)), dict(v_=f32(osg.YFaceField)), dict(w_=f32(osg.ZFaceField)), dict(t=[c, f32(osg.CenterField)]),
                   dict(G=[Gc, f32(osg.CenterField)])):
            a = dict(t=[c, d], u_=u, v_=v, w_=w, G=[Gc, Gd])
            a.update(kw)
            with pytest.raises(ValueError, match="one element type"):
                fn(a["t"], a["u_"], a["v_"], a["w_"], a["G"])
        for kw in (dict(u_=osg.XFaceField(grid, indices=window)), dict(w_=osg.ZFaceField(grid, indices=window)), dict(t=[c, new_c(indices=window)]),
                   dict(G=[Gc, new_c(indices=(slice(None), slice(None), 2))])):
            a = dict(t=[c, d], u_=u, v_=v, w_=w, G=[Gc, Gd])
            a.update(kw)
            with pytest.raises(NotImplementedError, match="z-windowed"):
                fn(a["t"], a["u_"], a["v_"], a["w_"], a["G"])
        # aliases, by identity
        with pytest.raises(ValueError, match="G of tracer 0 is tracer 0 itself"):
            fn([c], u, v, w, [c])
        with pytest.raises(ValueError, match="G of tracer 1 is tracer 0 itself"):
            fn([c, d], u, v, w, [Gc, new_c(data=c.data)])
        with pytest.raises(ValueError, match="G of tracer 1 and G of tracer 0 are one field"):
            fn([c, d], u, v, w, [Gc, Gc])
        # a halo narrower than (3, 3, 1), one direction at a time
        for halo in ((2, 3, 1), (3, 2, 1), (3, 3, 0), (1, 1, 1)):
            thin = _grid(osg, *halo)
            with pytest.raises(ValueError, match=rf"the halo must be at least \(3, 3, 1\) \(halo \({halo[0]}, {halo[1]}, {halo[2]}\)\)"):
                fn([new_c(thin)], osg.XFaceField(thin), osg.YFaceField(thin), osg.ZFaceField(thin), [new_c(thin)])
        # a latitude band
        band = _grid(osg, topology=(osg.PeriodicTopology, osg.FullyConnected, osg.Bounded), global_size=(8, 12, 3), jrange=(1, 6))
        with pytest.raises(NotImplementedError, match="latitude-band grids are not handled: the rows Ny \\+ 1 .. Ny \\+ 3 of a band are exchanged"):
            fn([new_c(band)], osg.XFaceField(band), osg.YFaceField(band), osg.ZFaceField(band), [new_c(band)])
    # out=None allocates only after the tracers are known to be Center fields
    with pytest.raises(TypeError, match=r"tracer 0 must be a Field at \(Center, Center, Center\)"):
        osg.weno_tracer_advection_tendency([u], u, v, w)
    with pytest.raises(TypeError, match="tracer 0 must be a Field"):
        osg.weno_tracer_advection_tendency([c.data], u, v, w)
    # the centred entry point keeps refusing what it refused
    with pytest.raises(NotImplementedError, match="scheme 'weno5' is not built"):
        osg.tracer_advection_plan([c], u, v, w, [Gc], scheme="weno5")


def test_build_and_documents_name_the_library():
    """the version script exports the two names, the kernel header is a prerequisite of every object, and
    the argument-check program is a stand-alone one with the sanitizer build line in its header, naming the sources it links"""
    from test_abi import ROOT
    mk = open(os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc", "Makefile")).read()
    vs = open(os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc", "weno.map")).read()
    assert all(n in vs for n in NAMES) and "local: *;" in vs
    tool = open(os.path.join(ROOT, "tools", "tracer_argcheck.cpp")).read()                    # one program over the three tracer calls
    assert "int main()" in tool and "-Xarch_host -fsanitize=address,undefined" in tool
    assert "csrc/tpg_weno.hip" in tool and "tpg_weno_tracer_advection_tendency" in tool
    # the library's file and the kernel header it includes, together
    csrc = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
    hip = open(os.path.join(csrc, "tpg_weno.hip")).read()
    assert '#include "tpg_weno_tracer_kernel.hpp"' in hip and "__global__" not in hip
    src = hip + open(os.path.join(csrc, "tpg_weno_tracer_kernel.hpp")).read()
    assert "tpg_advection.hip\"" not in src and '#include "tpg_operator.hpp"' in src
    assert "tpg_weno_tracer_kernel.hpp" in [ln for ln in mk.split("\n") if ln.startswith("HDRS")][0].split()
