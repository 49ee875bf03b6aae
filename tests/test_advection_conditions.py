"""Host-side tests of the tracer advection tendency (no GPU): the export list of libtripolar_hip_advection.so, every argument error of
tpg_tracer_advection_tendency (status and message; every call below fails in validation, none reaches a launch, the pointers are fabricated
and never dereferenced), every refusal of the Python layer on host-only grid records, and the loader."""
import ctypes as C

import pytest

from test_barotropic_conditions import _host_grid

NAMES = ["tpg_advection_last_error", "tpg_tracer_advection_tendency"]
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


def _call(lib, c=None, g=None, n=2, shared=None, n_cc=None, scheme=0, geom=G, ft=1, tables=True):
    c = [TRACER(q) for q in range(max(n, 1))] if c is None else c
    g = [TEND(q) for q in range(max(n, 1))] if g is None else g
    s = dict(u=U, v=V, w=W, dy=DY, dx=DX, az=AZ, dz=DZ)
    s.update(shared or {})
    ct, gt = (_table(c), _table(g)) if tables is True else tables
    return lib.tpg_tracer_advection_tendency(ct, gt, n, s["u"], s["v"], s["w"], s["dy"], s["dx"], s["az"], s["dz"], n_cc, 0.0, scheme, *geom, ft,
                                             None)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import declared_symbols, exported_symbols
    osg._lib.advection_lib()
    assert declared_symbols("tripolar_hip_advection.h") == NAMES == exported_symbols(osg._lib.ADVECTION_LIB_PATH) == sorted(osg._lib.ADVECTION_SIGNATURES)


def test_argument_errors_without_device_work(osg):
    lib = osg._lib.advection_lib()
    err = lambda: lib.tpg_advection_last_error().decode()
    # 1. the geometry
    assert _call(lib, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _call(lib, geom=(49, 40, 3, 4, 4, 4)) == -2
    assert _call(lib, geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert _call(lib, geom=(48, 40, 3, 4, 4, -1)) == -1 and err().startswith("invalid size")
    # 2. the scheme: only centered, second order, is built (checked before the tables are looked at)
    for scheme in (1, 5, -1):
        assert _call(lib, scheme=scheme) == -5 and err() == f"advection scheme {scheme} is not built (TPG_ADVECTION_CENTERED2 = 0 is)"
    # 3. the number of tracers
    assert _call(lib, n=0) == -1 and err() == "no tracers (nfields = 0)"
    assert _call(lib, n=-3) == -1 and err() == "no tracers (nfields = -3)"
    assert _call(lib, n=17) == -1 and err() == "17 tracers: at most TPG_MAX_FIELDS = 16 in one call"
    assert _call(lib, n=16, shared=dict(u=None)) == -1 and err() == "null u, v or w"     # 16 are accepted
    # 4. the tables and their entries
    assert _call(lib, tables=(None, _table([TEND(0), TEND(1)]))) == -1 and err() == "null table of tracers or of tendencies"
    assert _call(lib, tables=(_table([TRACER(0), TRACER(1)]), None)) == -1 and err() == "null table of tracers or of tendencies"
    assert _call(lib, c=[TRACER(0), None, TRACER(2)], n=3) == -1 and err() == "null tracer 1"
    assert _call(lib, g=[TEND(0), TEND(1), None], n=3) == -1 and err() == "null G of tracer 2"
    # 5. the velocities and the metrics
    for name in ("u", "v", "w"):
        assert _call(lib, shared={name: None}) == -1 and err() == "null u, v or w"
    for name in ("dy", "dx", "az", "dz"):
        assert _call(lib, shared={name: None}) == -1 and err() == "null dy_fc, dx_cf, az_cc or dz_c"
    # 6. alignment: to the element type, Float64 and Float32, and the count plane to int32
    assert _call(lib, c=[TRACER(0), TRACER(1) + 4]) == -1 and err() == "tracer 1: pointer not aligned to its element type"
    assert _call(lib, c=[TRACER(0), TRACER(1) + 2], ft=0) == -1 and err() == "tracer 1: pointer not aligned to its element type"
    assert _call(lib, g=[TEND(0) + 4, TEND(1)]) == -1 and err() == "G of tracer 0: pointer not aligned to its element type"
    for name in ("u", "v", "w"):
        assert _call(lib, shared={name: BASE + 3 * PARENT + 4}) == -1 and err() == "u, v or w pointer not aligned to its element type"
    for name, at in (("dy", DY), ("dx", DX), ("az", AZ), ("dz", DZ)):
        assert _call(lib, shared={name: at + 4}) == -1 and err() == "dy_fc, dx_cf, az_cc or dz_c pointer not aligned to its element type"
        assert _call(lib, shared={name: at + 2}, ft=0) == -1 and err() == "dy_fc, dx_cf, az_cc or dz_c pointer not aligned to its element type"
    assert _call(lib, n_cc=N + 2) == -1 and err() == "count plane pointer not aligned to int32"
    # 7. the overlaps: any G against any tracer, u, v, w and another G -- identical, one element inside from either side
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
    # 8. the halo the stencil needs, one direction at a time, both types
    for geom in ((48, 40, 3, 0, 4, 4), (48, 40, 3, 4, 0, 4), (48, 40, 3, 4, 4, 0)):
        for ft in (0, 1):
            assert _call(lib, geom=geom, ft=ft, n_cc=N) == -5 and "Hx >= 1, Hy >= 1 and Hz >= 1 needed" in err() and str(geom[3:]).replace(" ", "") in err()
    # 9. more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    big = [1 << 44, 2 << 44]
    assert _call(lib, c=big, g=[3 << 44, 4 << 44], shared=dict(u=5 << 44, v=6 << 44, w=7 << 44), geom=(65536, 32768, 1, 1, 1, 1), ft=0) == -5
    assert "32-bit" in err()


def test_python_refusals(osg):
    import torch
    for name in ("tracer_advection_tendency", "tracer_advection_plan", "TracerAdvectionPlan"):
        assert hasattr(osg, name), name
    for name in ("advection_lib", "check_advection", "ADVECTION_SIGNATURES", "ADVECTION_LIB_PATH", "TPG_ADVECTION_CENTERED2"):
        assert hasattr(osg._lib, name), name
    grid, other = _host_grid(osg), _host_grid(osg)
    new_c = lambda g=grid, **kw: osg.CenterField(g, **kw)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    c, d, Gc, Gd = new_c(), new_c(), new_c(), new_c()
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))
    window = (slice(None), slice(None), range(1, 3))
    for fn in (osg.tracer_advection_plan, lambda t, u_, v_, w_, G, **kw: osg.tracer_advection_tendency(t, u_, v_, w_, out=G, **kw)):
        with pytest.raises(TypeError, match="no tracers"):
            fn([], u, v, w, [])
        with pytest.raises(TypeError, match=r"lists of one length \(2, 1\)"):
            fn([c, d], u, v, w, [Gc])
        with pytest.raises(NotImplementedError, match="scheme 'weno5' is not built"):
            fn([c], u, v, w, [Gc], scheme="weno5")
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
        # a halo smaller than 1
        flat = osg.OrthogonalSphericalShellGrid(
            architecture=None, Nx=8, Ny=6, Nz=3, Hx=1, Hy=1, Hz=0, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10, dtype=torch.float64)},
            z_faces=torch.zeros(4), z_centers=torch.zeros(3), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
            topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=torch.float64, z_spec=(-1, 0))
        with pytest.raises(ValueError, match=r"every halo must be at least 1 \(halo \(1, 1, 0\)\)"):
            fn([new_c(flat)], osg.XFaceField(flat), osg.YFaceField(flat), osg.ZFaceField(flat), [new_c(flat)])
        # a latitude band
        band = osg.OrthogonalSphericalShellGrid(
            architecture=None, Nx=8, Ny=6, Nz=3, Hx=1, Hy=1, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10, dtype=torch.float64)},
            z_faces=torch.zeros(6), z_centers=torch.zeros(5), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
            topology=(osg.PeriodicTopology, osg.FullyConnected, osg.Bounded), dtype=torch.float64, z_spec=(-1, 0), global_size=(8, 12, 3),
            jrange=(1, 6))
        with pytest.raises(NotImplementedError, match="row Ny \\+ 1 of a band is the exchanged halo row, and the band path .* is not tested yet"):
            fn([new_c(band)], osg.XFaceField(band), osg.YFaceField(band), osg.ZFaceField(band), [new_c(band)])
    # out=None allocates only after the tracers are known to be Center fields
    with pytest.raises(TypeError, match=r"tracer 0 must be a Field at \(Center, Center, Center\)"):
        osg.tracer_advection_tendency([u], u, v, w)
    with pytest.raises(TypeError, match="tracer 0 must be a Field"):
        osg.tracer_advection_tendency([c.data], u, v, w)
