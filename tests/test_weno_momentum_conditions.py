"""Host-side tests of the momentum advection tendency with the WENO5-upwinded vorticity term (no GPU): the export list of
libtripolar_hip_weno_momentum.so, every argument error of tpg_weno_momentum_advection_tendency in the order the header gives (status and
message; every call below fails in validation, none reaches a launch, the pointers are fabricated and never dereferenced), every refusal of
the Python layer on host-only grid records, the refusals of the enstrophy-conserving call that must stay as they are, the loader, and the
names the build is made of."""
import os

import pytest

NAMES = ["tpg_weno_momentum_advection_tendency", "tpg_weno_momentum_last_error"]
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
BUILT_NAME = "VectorInvariant(vorticity_scheme=WENO(order=5), vertical_scheme=EnergyConserving(), vorticity_stencil=DefaultStencil())"


def _call(lib, n_fc=None, n_cf=None, geom=G, ft=1, **over):
    s = dict(u=U, v=V, w=W, Gu=GU, Gv=GV, **AT)
    s.update(over)
    return lib.tpg_weno_momentum_advection_tendency(s["u"], s["v"], s["w"], s["Gu"], s["Gv"], *(s[k] for k in METRICS), n_fc, n_cf, 0.0,
                                                    *geom, ft, None)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import ROOT, declared_symbols, exported_symbols
    L = osg._lib
    L.weno_momentum_lib()
    assert sorted(declared_symbols("tripolar_hip_weno_momentum.h")) == NAMES == sorted(exported_symbols(L.WENO_MOMENTUM_LIB_PATH)) \
        == sorted(L.WENO_MOMENTUM_SIGNATURES)


def test_argument_errors_without_device_work(osg):
    lib = osg._lib.weno_momentum_lib()
    err = lambda: lib.tpg_weno_momentum_last_error().decode()     # noqa: E731
    # 1. the geometry
    assert _call(lib, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _call(lib, geom=(49, 40, 3, 4, 4, 4)) == -2
    assert _call(lib, geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert _call(lib, geom=(48, 40, 3, 4, 4, -1)) == -1 and err().startswith("invalid size")
    # 2. the velocities, the tendencies, the metrics (each checked before what follows it)
    for name in ("u", "v", "w"):
        assert _call(lib, Gu=None, **{name: None}) == -1 and err() == "null u, v or w"
    for name in ("Gu", "Gv"):
        assert _call(lib, dx_fc=None, **{name: None}) == -1 and err() == "null Gu or Gv"
    for name in METRICS:
        assert _call(lib, n_fc=NFC, **{name: None}) == -1 and err() == NULL_METRIC
    # 3. one count plane without the other
    assert _call(lib, n_fc=NFC, u=U + 4) == -1 and err() == "the count planes n_fc and n_cf are given together or not at all (n_cf is null)"
    assert _call(lib, n_cf=NCF) == -1 and err() == "the count planes n_fc and n_cf are given together or not at all (n_fc is null)"
    # 4. alignment: to the element type, Float64 and Float32, and the count planes to int32
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
    # 5. the overlaps: Gu and Gv against u, v, w and each other -- identical, one element inside from either side
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
    # u, v and w are only read: they may be one array
    assert _call(lib, geom=h0, u=BASE, v=BASE, w=BASE) == -5
    # 6. the halo the stencil needs, one direction at a time, both types: the message names the stencil and the halo passed
    for geom in ((48, 40, 3, 2, 4, 4), (48, 40, 3, 4, 2, 4), (48, 40, 3, 4, 4, 0), (48, 40, 3, 1, 1, 1)):
        for ft in (0, 1):
            assert _call(lib, geom=geom, ft=ft, n_fc=NFC, n_cf=NCF) == -5
            assert "Z[i, j-2..j+3] and Z[i-2..i+3, j]" in err() and "Hx >= 3, Hy >= 3 and Hz >= 1 needed" in err()
            assert "(halo " + str(geom[3:]).replace(" ", "") + ")" in err()
    assert _call(lib, geom=(48, 40, 3, 3, 3, 1), u=None) == -1     # the minimum halo passes the halo check (and is refused for what comes before)
    # 7. more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    assert _call(lib, geom=(65536, 32768, 1, 3, 3, 1), ft=0, u=1 << 44, v=2 << 44, w=3 << 44, Gu=4 << 44, Gv=5 << 44) == -5
    assert "32-bit" in err()


def test_the_enstrophy_call_still_refuses_every_other_scheme(osg):
    """tpg_momentum_advection_tendency builds scheme 0 only, and momentum_advection_plan(scheme="weno") raises what it raised: the WENO
    vorticity term is a call of its own"""
    lib = osg._lib.momentum_lib()
    for scheme in (1, 2, 5, -1):
        rc = lib.tpg_momentum_advection_tendency(U, V, W, GU, GV, *(AT[k] for k in METRICS), None, None, 0.0, scheme, *G, 1, None)
        assert rc == -5 and lib.tpg_momentum_last_error().decode() == f"momentum advection scheme {scheme} is not built (TPG_MOMENTUM_ENSTROPHY_CONSERVING = 0 is)"
    grid = _grid(osg)
    with pytest.raises(NotImplementedError, match="scheme 'weno' is not built \\('enstrophy_conserving' is"):
        osg.momentum_advection_plan(osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid),
                                    scheme="weno")


def _grid(osg, halo=(3, 3, 1), dtype=None, **kw):
    """an OrthogonalSphericalShellGrid record with host tensors: enough for the checks that touch no device"""
    import torch
    dtype = dtype or torch.float64
    Hx, Hy, Hz = halo
    args = dict(architecture=None, Nx=8, Ny=6, Nz=3, Hx=Hx, Hy=Hy, Hz=Hz, Lz=1.0, arrays={"lambda_cc": torch.zeros(6 + 2 * Hy, 8 + 2 * Hx, dtype=dtype)},
                z_faces=torch.zeros(4 + 2 * Hz), z_centers=torch.zeros(3 + 2 * Hz), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
                topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=dtype, z_spec=(-1, 0))
    args.update(kw)
    return osg.OrthogonalSphericalShellGrid(**args)


def test_python_refusals(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd import weno_momentum as wm
    for name in ("weno_momentum_advection_tendency", "weno_momentum_advection_plan", "WenoMomentumAdvectionPlan", "VectorInvariant",
                 "EnergyConserving", "DefaultStencil", "VelocityStencil", "WENOVectorInvariant", "WENO", "Centered"):
        assert hasattr(osg, name), name
    for name in ("weno_momentum_lib", "check_weno_momentum", "WENO_MOMENTUM_SIGNATURES", "WENO_MOMENTUM_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    from orthogonalsphericalshellgrids.jl_amd._operator_plan import OperatorPlan
    assert issubclass(osg.WenoMomentumAdvectionPlan, OperatorPlan)
    assert wm.BUILT == osg.VectorInvariant(vorticity_scheme=osg.WENO(order=5), vertical_scheme=osg.EnergyConserving(),
                                           vorticity_stencil=osg.DefaultStencil())
    grid, other = _grid(osg), _grid(osg)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))       # noqa: E731
    window = (slice(None), slice(None), range(1, 3))
    # the function of the reference's drivers: its message names the three missing pieces and what is built
    for order in (5, 7):
        with pytest.raises(NotImplementedError) as e:
            osg.WENOVectorInvariant(vorticity_order=order)
        assert all(piece in str(e.value) for piece in ("upwinded divergence flux", "upwinded kinetic-energy gradient", "VelocityStencil smoothness",
                                                       BUILT_NAME))
    with pytest.raises(NotImplementedError):
        osg.WENOVectorInvariant()
    for fn in (osg.weno_momentum_advection_plan, lambda u_, v_, w_, a, b, **kw: osg.weno_momentum_advection_tendency(u_, v_, w_, out=(a, b), **kw)):
        # the schemes: checked first, each message names what is built
        with pytest.raises(NotImplementedError, match="enstrophy-conserving vorticity term is momentum_advection_plan's") as e:
            fn(u, v, w, Gu, Gv, scheme=osg.VectorInvariant())
        assert BUILT_NAME in str(e.value)
        for order in (3, 7, 9):
            with pytest.raises(NotImplementedError, match=f"WENO of order {order} is not built") as e:
                fn(u, v, w, Gu, Gv, scheme=osg.VectorInvariant(vorticity_scheme=osg.WENO(order=order)))
            assert BUILT_NAME in str(e.value)
        with pytest.raises(NotImplementedError, match="VelocityStencil smoothness is not built") as e:
            fn(u, v, w, Gu, Gv, scheme=osg.VectorInvariant(vorticity_scheme=osg.WENO(order=5), vorticity_stencil=osg.VelocityStencil()))
        assert BUILT_NAME in str(e.value)
        for scheme in ("weno", "enstrophy_conserving", None, osg.WENO(order=5),
                       osg.VectorInvariant(vorticity_scheme=osg.WENO(order=5), vertical_scheme=osg.WENO(order=5)),
                       osg.VectorInvariant(vorticity_scheme=osg.Centered())):
            with pytest.raises(NotImplementedError, match="is not built") as e:
                fn(u, v, w, Gu, Gv, scheme=scheme)
            assert BUILT_NAME in str(e.value)
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
        # a halo thinner than (3, 3, 1), one direction at a time: the message names the halo passed
        for halo in ((2, 3, 1), (3, 2, 1), (3, 3, 0), (1, 1, 1)):
            thin = _grid(osg, halo)
            with pytest.raises(ValueError, match=r"the halo must be at least \(3, 3, 1\) \(halo \(%d, %d, %d\)\)" % halo):
                fn(osg.XFaceField(thin), osg.YFaceField(thin), osg.ZFaceField(thin), osg.XFaceField(thin), osg.YFaceField(thin))
        # a latitude band
        band = _grid(osg, topology=(osg.PeriodicTopology, osg.FullyConnected, osg.Bounded), global_size=(8, 12, 3), jrange=(1, 6))
        with pytest.raises(NotImplementedError, match="rows Ny \\+ 1 .. Ny \\+ 3 of a band are exchanged halo rows, and the band path .* is not tested yet"):
            fn(osg.XFaceField(band), osg.YFaceField(band), osg.ZFaceField(band), osg.XFaceField(band), osg.YFaceField(band))
    # out=None allocates only after u is known to be an XFace field
    with pytest.raises(TypeError, match=r"u must be a Field at \(Face, Center, Center\)"):
        osg.weno_momentum_advection_tendency(v, v, w)
    with pytest.raises(TypeError, match="u must be a Field"):
        osg.weno_momentum_advection_tendency(u.data, v, w)


def test_missing_library_fails_loudly(osg, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the plan raises: it computes nothing some other way"""
    missing = str(tmp_path / os.path.basename(osg._lib.WENO_MOMENTUM_LIB_PATH))
    monkeypatch.setattr(osg._lib, "_weno_momentum", None)
    monkeypatch.setattr(osg._lib, "WENO_MOMENTUM_LIB_PATH", missing)
    grid = _grid(osg)
    with pytest.raises(ImportError, match="only backend"):
        osg.weno_momentum_advection_plan(osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid))


def test_the_build_names_the_library_the_map_and_the_argcheck_tool():
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "tpg_weno_face.hpp" in make
    text = open(os.path.join(csrc, "weno_momentum.map")).read()
    assert all(n in text for n in NAMES) and "local: *;" in text
    # W5 has one definition in the tree: the shared header, included by both kernels (each lives in a header of its own, which its
    # libraries' files include)
    for src in ("tpg_weno_tracer_kernel.hpp", "tpg_weno_vorticity_kernel.hpp"):
        body = open(os.path.join(csrc, src)).read()
        assert '#include "tpg_weno_face.hpp"' in body and "T weno_face(" not in body
    assert open(os.path.join(csrc, "tpg_weno_face.hpp")).read().count("T weno_face(") == 1
    for src in ("tpg_weno.hip", "tpg_weno_xyz.hip"):                 # the tracer libraries' files reach it through their kernel header
        body = open(os.path.join(csrc, src)).read()
        assert '#include "tpg_weno_tracer_kernel.hpp"' in body and "T weno_face(" not in body
    body = open(os.path.join(csrc, "tpg_weno_momentum.hip")).read()
    assert '#include "tpg_weno_vorticity_kernel.hpp"' in body and "T weno_face(" not in body and "__global__" not in body
    assert "tpg_weno_vorticity_kernel.hpp" in [ln for ln in make.split("\n") if ln.startswith("HDRS")][0].split()
    assert "TPG_WVI" not in body and "TPG_WMOM" not in open(os.path.join(csrc, "tpg_weno_vorticity_kernel.hpp")).read()
    tool = open(os.path.join(ROOT, "tools", "momentum_argcheck.cpp")).read()                               # one program over both momentum calls
    assert "-Xarch_host -fsanitize=address,undefined" in tool and "int main()" in tool and "tpg_weno_momentum_advection_tendency" in tool
    assert "tpg_momentum_advection_tendency" in tool and "csrc/tpg_momentum.hip" in tool and "csrc/tpg_weno_momentum.hip" in tool
