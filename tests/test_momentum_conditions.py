"""Host-side tests of the momentum advection tendency (no GPU): the export list of libtripolar_hip_momentum.so, every argument error of
tpg_momentum_advection_tendency (status and message; every call below fails in validation, none reaches a launch, the pointers are fabricated
and never dereferenced), every refusal of the Python layer on host-only grid records, the face-spacing helper, and the loader."""

import pytest

from test_barotropic_conditions import _host_grid

NAMES = ["tpg_momentum_advection_tendency", "tpg_momentum_last_error"]
G = (48, 40, 3, 4, 4, 4)                                           # Nx, Ny, Nz, Hx, Hy, Hz
PLANE = 56 * 48 * 8
PARENT, WPARENT = PLANE * 11, PLANE * 12                           # bytes of a Float64 parent of u, v, Gu, Gv (Nz + 2Hz planes) and of w (one more)
BASE, FAR = 1 << 30, 1 << 40
U, V, W = BASE, BASE + PARENT, BASE + 2 * PARENT
GU, GV = FAR, FAR + 3 * PARENT
METRICS = ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff", "dz_f")
AT = {name: (q + 1) << 20 for q, name in enumerate(METRICS)}
NFC, NCF = 20 << 20, 21 << 20
NULL_METRIC = "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f"
OFF_METRIC = "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f pointer not aligned to its element type"


def _call(lib, n_fc=None, n_cf=None, scheme=0, geom=G, ft=1, **over):
    s = dict(u=U, v=V, w=W, Gu=GU, Gv=GV, **AT)
    s.update(over)
    return lib.tpg_momentum_advection_tendency(s["u"], s["v"], s["w"], s["Gu"], s["Gv"], *(s[k] for k in METRICS), n_fc, n_cf, 0.0, scheme,
                                               *geom, ft, None)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import declared_symbols, exported_symbols
    osg._lib.momentum_lib()
    assert sorted(declared_symbols("tripolar_hip_momentum.h")) == NAMES == sorted(exported_symbols(osg._lib.MOMENTUM_LIB_PATH)) == sorted(osg._lib.MOMENTUM_SIGNATURES)


def test_argument_errors_without_device_work(osg):
    lib = osg._lib.momentum_lib()
    err = lambda: lib.tpg_momentum_last_error().decode()          # noqa: E731
    # 1. the geometry
    assert _call(lib, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _call(lib, geom=(49, 40, 3, 4, 4, 4)) == -2
    assert _call(lib, geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert _call(lib, geom=(48, 40, 3, 4, 4, -1)) == -1 and err().startswith("invalid size")
    # 2. the scheme: only the enstrophy-conserving one is built (checked before any pointer is looked at)
    for scheme in (1, 5, -1):
        assert _call(lib, scheme=scheme, u=None) == -5
        assert err() == f"momentum advection scheme {scheme} is not built (TPG_MOMENTUM_ENSTROPHY_CONSERVING = 0 is)"
    # 3. the velocities, the tendencies, the metrics
    for name in ("u", "v", "w"):
        assert _call(lib, Gu=None, **{name: None}) == -1 and err() == "null u, v or w"
    for name in ("Gu", "Gv"):
        assert _call(lib, dx_fc=None, **{name: None}) == -1 and err() == "null Gu or Gv"
    for name in METRICS:
        assert _call(lib, n_fc=NFC, **{name: None}) == -1 and err() == NULL_METRIC
    # 4. one count plane without the other
    assert _call(lib, n_fc=NFC, u=U + 4) == -1 and err() == "the count planes n_fc and n_cf are given together or not at all (n_cf is null)"
    assert _call(lib, n_cf=NCF) == -1 and err() == "the count planes n_fc and n_cf are given together or not at all (n_fc is null)"
    # 5. alignment: to the element type, Float64 and Float32, and the count planes to int32
    for name in ("u", "v", "w"):
        assert _call(lib, **{name: BASE + 3 * PARENT + 4}) == -1 and err() == "u, v or w pointer not aligned to its element type"
        assert _call(lib, ft=0, **{name: BASE + 3 * PARENT + 2}) == -1 and err() == "u, v or w pointer not aligned to its element type"
    for name, at in (("Gu", GU), ("Gv", GV)):
        assert _call(lib, **{name: at + 4}) == -1 and err() == "Gu or Gv pointer not aligned to its element type"
        assert _call(lib, ft=0, **{name: at + 2}) == -1 and err() == "Gu or Gv pointer not aligned to its element type"
    for name in METRICS:
        assert _call(lib, **{name: AT[name] + 4}) == -1 and err() == OFF_METRIC
        assert _call(lib, ft=0, **{name: AT[name] + 2}) == -1 and err() == OFF_METRIC
    assert _call(lib, n_fc=NFC + 2, n_cf=NCF) == -1 and err() == "count plane pointer not aligned to int32"
    assert _call(lib, n_fc=NFC, n_cf=NCF + 2) == -1 and err() == "count plane pointer not aligned to int32"
    # 6. the overlaps: Gu and Gv against u, v, w and each other -- identical, one element inside from either side
    away = dict(u=3 * FAR, v=4 * FAR, w=5 * FAR)
    for shift in (0, 8, -8, PARENT - 8, 8 - PARENT):
        for out in ("Gu", "Gv"):
            for name in ("u", "v"):
                assert _call(lib, **{**away, name: BASE, out: BASE + shift}) == -1 and err().startswith(f"{out} overlaps {name} ("), (out, name, shift)
        assert _call(lib, Gv=GU + shift) == -1 and err() == "Gv overlaps Gu", shift
    for shift in (0, 8, -8, WPARENT - 8, 8 - PARENT):              # w's parent is one level longer
        for out in ("Gu", "Gv"):
            assert _call(lib, **{**away, "w": BASE, out: BASE + shift}) == -1 and err().startswith(f"{out} overlaps w ("), (out, shift)
    # exact: an output right behind or right in front of an array is no overlap (the call goes on to refuse Hz = 0), one element nearer is
    h0 = (48, 40, 3, 4, 4, 0)
    p0, w0 = PLANE * 3, PLANE * 4
    for out in ("Gu", "Gv"):
        for shift, status in ((p0, -5), (p0 - 8, -1), (-p0, -5), (8 - p0, -1)):
            assert _call(lib, geom=h0, **{**away, "u": BASE, out: BASE + shift}) == status, (out, shift)
            assert err().startswith(f"{out} overlaps u" if status == -1 else "the rule reads")
        for shift, status in ((w0, -5), (w0 - 8, -1), (-p0, -5), (8 - p0, -1)):
            assert _call(lib, geom=h0, **{**away, "w": BASE, out: BASE + shift}) == status, (out, shift)
            assert err().startswith(f"{out} overlaps w" if status == -1 else "the rule reads")
    for shift, status in ((p0, -5), (p0 - 8, -1), (-p0, -5), (8 - p0, -1)):
        assert _call(lib, geom=h0, Gv=GU + shift) == status and err().startswith("Gv overlaps Gu" if status == -1 else "the rule reads"), shift
    # u, v and w are only read: they may be one array
    assert _call(lib, geom=h0, u=BASE, v=BASE, w=BASE) == -5
    # 7. the halo the stencil needs, one direction at a time, both types
    for geom in ((48, 40, 3, 0, 4, 4), (48, 40, 3, 4, 0, 4), (48, 40, 3, 4, 4, 0)):
        for ft in (0, 1):
            assert _call(lib, geom=geom, ft=ft, n_fc=NFC, n_cf=NCF) == -5
            assert "Hx >= 1, Hy >= 1 and Hz >= 1 needed" in err() and str(geom[3:]).replace(" ", "") in err()
    # 8. more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    assert _call(lib, geom=(65536, 32768, 1, 1, 1, 1), ft=0, u=1 << 44, v=2 << 44, w=3 << 44, Gu=4 << 44, Gv=5 << 44) == -5
    assert "32-bit" in err()


def test_python_refusals(osg):
    import torch
    for name in ("momentum_advection_tendency", "momentum_advection_plan", "MomentumAdvectionPlan", "z_all_face_spacings"):
        assert hasattr(osg, name), name
    for name in ("momentum_lib", "check_momentum", "MOMENTUM_SIGNATURES", "MOMENTUM_LIB_PATH", "TPG_MOMENTUM_ENSTROPHY_CONSERVING"):
        assert hasattr(osg._lib, name), name
    grid, other = _host_grid(osg), _host_grid(osg)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))       # noqa: E731
    window = (slice(None), slice(None), range(1, 3))
    for fn in (osg.momentum_advection_plan, lambda u_, v_, w_, a, b, **kw: osg.momentum_advection_tendency(u_, v_, w_, out=(a, b), **kw)):
        with pytest.raises(NotImplementedError, match="scheme 'weno' is not built"):
            fn(u, v, w, Gu, Gv, scheme="weno")
        # locations
        with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
            fn(v, v, w, Gu, Gv)
        with pytest.raises(TypeError, match=r"v must be a Field at \(Center, Face, Center\)"):
            fn(u, c, w, Gu, Gv)
        with pytest.raises(TypeError, match=r"w must be a Field at \(Center, Center, Face\)"):
            fn(u, v, c, Gu, Gv)
        with pytest.raises(TypeError, match="w must be a Field"):
            fn(u, v, w.data, Gu, Gv)
        with pytest.raises(TypeError, match=r"Gu must be a Field at \(Face, Center, Center\)"):
            fn(u, v, w, Gv, Gv)
        with pytest.raises(TypeError, match=r"Gv must be a Field at \(Center, Face, Center\)"):
            fn(u, v, w, Gu, osg.XFaceField(grid))
        with pytest.raises(TypeError, match="Gu must be a Field"):
            fn(u, v, w, Gu.data, Gv)
        # one grid, one type, no z-window: for every field of the call
        base = dict(u=u, v=v, w=w, Gu=Gu, Gv=Gv)
        makers = dict(u=osg.XFaceField, v=osg.YFaceField, w=osg.ZFaceField, Gu=osg.XFaceField, Gv=osg.YFaceField)
        for name in ("v", "w", "Gu", "Gv"):
            a = dict(base, **{name: makers[name](other)})
            with pytest.raises(ValueError, match="one grid"):
                fn(*a.values())
            a = dict(base, **{name: f32(makers[name])})
            with pytest.raises(ValueError, match="one element type"):
                fn(*a.values())
        for name in makers:
            a = dict(base, **{name: makers[name](grid, indices=window)})
            with pytest.raises(NotImplementedError, match="z-windowed"):
                fn(*a.values())
        # aliases, by identity
        with pytest.raises(ValueError, match="Gu is u itself"):
            fn(u, v, w, u, Gv)
        with pytest.raises(ValueError, match="Gv is v itself"):
            fn(u, v, w, Gu, osg.YFaceField(grid, data=v.data))
        with pytest.raises(ValueError, match="Gu and Gv are one field"):
            fn(u, v, w, Gu, osg.YFaceField(grid, data=Gu.data))
        # a halo smaller than 1
        flat = osg.OrthogonalSphericalShellGrid(
            architecture=None, Nx=8, Ny=6, Nz=3, Hx=1, Hy=1, Hz=0, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10, dtype=torch.float64)},
            z_faces=torch.zeros(4), z_centers=torch.zeros(3), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
            topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=torch.float64, z_spec=(-1, 0))
        with pytest.raises(ValueError, match=r"every halo must be at least 1 \(halo \(1, 1, 0\)\)"):
            fn(osg.XFaceField(flat), osg.YFaceField(flat), osg.ZFaceField(flat), osg.XFaceField(flat), osg.YFaceField(flat))
        # a latitude band
        band = osg.OrthogonalSphericalShellGrid(
            architecture=None, Nx=8, Ny=6, Nz=3, Hx=1, Hy=1, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(8, 10, dtype=torch.float64)},
            z_faces=torch.zeros(6), z_centers=torch.zeros(5), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
            topology=(osg.PeriodicTopology, osg.FullyConnected, osg.Bounded), dtype=torch.float64, z_spec=(-1, 0), global_size=(8, 12, 3),
            jrange=(1, 6))
        with pytest.raises(NotImplementedError, match="row Ny \\+ 1 of a band is the exchanged halo row, and the band path .* is not tested yet"):
            fn(osg.XFaceField(band), osg.YFaceField(band), osg.ZFaceField(band), osg.XFaceField(band), osg.YFaceField(band))
    # out=None allocates only after u is known to be an XFace field
    with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
        osg.momentum_advection_tendency(v, v, w)
    with pytest.raises(TypeError, match="u must be a Field"):
        osg.momentum_advection_tendency(u.data, v, w)


@pytest.mark.parametrize("z", [(-1, 0), (-1000.0, 0.0), [-10.0, -6.0, -3.5, -1.7, -0.6, 0.0], [-7.0, -6.0, -2.5, -2.0, -0.125]], ids=str)
def test_all_face_spacings_extend_z_face_spacings(osg, z):
    """Nz + 1 values; the first Nz are z_face_spacings' bit for bit; the last is the spacing to the halo centre above the top face, which
    the grid's z coordinate extrapolates with the top cell's thickness; float64 arithmetic rounded once to the type asked for"""
    import numpy as np
    import torch
    Nz = len(z) - 1 if isinstance(z, list) else 7
    for dtype, npt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        grid = _host_grid(osg, dtype, z, Nz)
        for ask in (None, torch.float64, torch.float32):
            all_, some = osg.z_all_face_spacings(grid, ask), osg.z_face_spacings(grid, ask)
            assert all_.dtype == torch.float64 and all_.shape == (Nz + 1,) and some.shape == (Nz,)
            assert torch.equal(all_[:Nz].view(torch.int64), some.view(torch.int64))
        d = osg.z_all_face_spacings(grid).numpy()
        if isinstance(z, list):
            f = np.array(z)
            ext = np.concatenate([[f[0] - (f[1] - f[0])], f, [f[-1] + (f[-1] - f[-2])]])    # one halo face below and above
            want = np.float64(npt(np.diff(0.5 * (ext[1:] + ext[:-1]))))                     # differences of the Nz + 2 centres, rounded once
            assert f[-1] - f[-2] != f[-2] - f[-3] and want[Nz] != want[Nz - 1]
        else:
            want = np.full(Nz + 1, np.float64(npt((float(z[1]) - float(z[0])) / Nz)))
        assert np.array_equal(d, want)
