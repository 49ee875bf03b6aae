"""Host-side tests of the momentum advection tendency with upwinding in every term (no GPU): the export list of
libtripolar_hip_weno_vi.so, every argument error of tpg_weno_vi_momentum_advection_tendency in the order the header gives (status and
message; every call below fails in validation, none reaches a launch, the pointers are fabricated and never dereferenced), every refusal of
the Python layer on host-only grid records, the records, the refusals of the two older calls that must stay as they are, the loader, and the
names the build is made of."""
import os

import pytest

from test_weno_momentum_conditions import AT as _AT_F, BASE, FAR, G, GU, GV, NCF, NFC, PARENT, PLANE, U, V, W, WPARENT, _grid

NAMES = ["tpg_weno_vi_last_error", "tpg_weno_vi_momentum_advection_tendency"]
METRICS = ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff", "dz_c")
AT = {name: (q + 1) << 20 for q, name in enumerate(METRICS)}
NULL_METRIC = "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_c"
OFF_METRIC = "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_c pointer not aligned to its element type"
STENCIL = "u, v[i-3..i+3, j-3..j+3, k-3..k+3 within 0..Nz+1] and w[i-2..i+1, j], w[i, j-2..j+1]"
BUILT_NAME = ("VectorInvariant(vorticity_scheme=WENO(order=5), vorticity_stencil=DefaultStencil(), vertical_scheme=WENO(order=5), "
              "kinetic_energy_gradient_scheme=WENO(order=5), divergence_scheme=WENO(order=5), "
              "upwinding=OnlySelfUpwinding(cross_scheme=WENO(order=5)))")
OLD_BUILT_NAME = "VectorInvariant(vorticity_scheme=WENO(order=5), vertical_scheme=EnergyConserving(), vorticity_stencil=DefaultStencil())"


def _call(lib, n_fc=None, n_cf=None, geom=G, ft=1, **over):
    s = dict(u=U, v=V, w=W, Gu=GU, Gv=GV, **AT)
    s.update(over)
    return lib.tpg_weno_vi_momentum_advection_tendency(s["u"], s["v"], s["w"], s["Gu"], s["Gv"], *(s[k] for k in METRICS), n_fc, n_cf, 0.0,
                                                       *geom, ft, None)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import ROOT, declared_symbols, exported_symbols
    L = osg._lib
    L.weno_vi_lib()
    assert sorted(declared_symbols("tripolar_hip_weno_vi.h")) == NAMES == sorted(exported_symbols(L.WENO_VI_LIB_PATH)) == sorted(L.WENO_VI_SIGNATURES)


def test_argument_errors_without_device_work(osg):
    lib = osg._lib.weno_vi_lib()
    err = lambda: lib.tpg_weno_vi_last_error().decode()           # noqa: E731
    # 1. the geometry
    assert _call(lib, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _call(lib, geom=(49, 40, 3, 4, 4, 4)) == -2
    assert _call(lib, geom=(48, 40, 0, 4, 4, 4)) == -1 and err().startswith("invalid size")
    assert _call(lib, geom=(48, 40, 3, 4, 4, -1)) == -1 and err().startswith("invalid size")
    # 2. the velocities, the tendencies, the metrics and dz_c (each checked before what follows it)
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
    assert _call(lib, geom=h0, u=BASE, v=BASE, w=BASE) == -5       # u, v and w are only read: they may be one array
    # 6. the halo the stencil needs, one direction at a time, both types: the message names the stencil and the halo passed
    for geom in ((48, 40, 3, 2, 4, 4), (48, 40, 3, 4, 2, 4), (48, 40, 3, 4, 4, 0), (48, 40, 3, 1, 1, 1)):
        for ft in (0, 1):
            assert _call(lib, geom=geom, ft=ft, n_fc=NFC, n_cf=NCF) == -5
            assert err() == f"the rule reads {STENCIL}: Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo " + str(geom[3:]).replace(" ", "") + ")"
    assert _call(lib, geom=(48, 40, 3, 3, 3, 1), u=None) == -1     # the minimum halo passes the halo check (and is refused for what comes before)
    # 7. more work items than 32 bits index: refused by the plane check every entry point shares, or by the call's own
    assert _call(lib, geom=(65536, 32768, 1, 3, 3, 1), ft=0, u=1 << 44, v=2 << 44, w=3 << 44, Gu=4 << 44, Gv=5 << 44) == -5
    assert "32-bit" in err()


def test_the_older_calls_keep_their_messages_and_refuse_the_new_record(osg):
    """the shared host layer now names the spacing table of a call: the two older calls still say dz_f, word for word, and both refuse
    weno_vi.BUILT as they refused every scheme but their own"""
    from orthogonalsphericalshellgrids.jl_amd import weno_momentum as wm, weno_vi
    metrics_f = tuple(_AT_F)
    assert metrics_f[-1] == "dz_f"
    wlib, mlib = osg._lib.weno_momentum_lib(), osg._lib.momentum_lib()
    args = lambda **over: [{**dict(u=U, v=V, w=W, Gu=GU, Gv=GV), **_AT_F, **over}[k] for k in ("u", "v", "w", "Gu", "Gv", *metrics_f)]     # noqa: E731
    assert wlib.tpg_weno_momentum_advection_tendency(*args(dz_f=None), None, None, 0.0, *G, 1, None) == -1
    assert wlib.tpg_weno_momentum_last_error().decode() == "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f"
    assert mlib.tpg_momentum_advection_tendency(*args(dz_f=_AT_F["dz_f"] + 4), None, None, 0.0, 0, *G, 1, None) == -1
    assert mlib.tpg_momentum_last_error().decode() == "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f pointer not aligned to its element type"
    assert wm.BUILT == osg.VectorInvariant(vorticity_scheme=osg.WENO(order=5), vertical_scheme=osg.EnergyConserving(), vorticity_stencil=osg.DefaultStencil())
    assert wm.BUILT.kinetic_energy_gradient_scheme is None and wm.BUILT.divergence_scheme is None and wm.BUILT.upwinding is None
    assert wm.BUILT != weno_vi.BUILT and osg.VectorInvariant() == osg.VectorInvariant(osg.EnstrophyConserving(), osg.EnergyConserving(), osg.DefaultStencil())
    grid = _grid(osg)
    f = lambda: (osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid))      # noqa: E731
    with pytest.raises(NotImplementedError, match="is not built") as e:
        osg.weno_momentum_advection_plan(*f(), scheme=weno_vi.BUILT)
    assert OLD_BUILT_NAME in str(e.value) and "weno_vi_momentum_advection_plan" in str(e.value)
    with pytest.raises(NotImplementedError, match="is not built"):
        osg.weno_momentum_advection_tendency(*f()[:3], scheme=weno_vi.BUILT)
    with pytest.raises(NotImplementedError, match="is not built \\('enstrophy_conserving' is"):
        osg.momentum_advection_plan(*f(), scheme=weno_vi.BUILT)


def test_the_records(osg):
    from orthogonalsphericalshellgrids.jl_amd import weno_vi
    assert osg.OnlySelfUpwinding() == osg.OnlySelfUpwinding(cross_scheme=osg.Centered()) != osg.OnlySelfUpwinding(cross_scheme=osg.WENO(order=5))
    vi = osg.VectorInvariant()
    assert (vi.kinetic_energy_gradient_scheme, vi.divergence_scheme, vi.upwinding) == (None, None, None)
    assert weno_vi.BUILT == osg.VectorInvariant(vorticity_scheme=osg.WENO(order=5), vorticity_stencil=osg.DefaultStencil(),
                                                vertical_scheme=osg.WENO(order=5), kinetic_energy_gradient_scheme=osg.WENO(order=5),
                                                divergence_scheme=osg.WENO(order=5),
                                                upwinding=osg.OnlySelfUpwinding(cross_scheme=osg.WENO(order=5)))
    assert hash(weno_vi.BUILT) == hash(weno_vi.BUILT)              # a frozen record
    for order in (5, 7):                                           # the drivers' constructor still raises, and says what is built where
        with pytest.raises(NotImplementedError) as e:
            osg.WENOVectorInvariant(vorticity_order=order)
        assert all(piece in str(e.value) for piece in ("upwinded divergence flux", "upwinded kinetic-energy gradient", "VelocityStencil smoothness",
                                                       OLD_BUILT_NAME, "weno_vi.BUILT", "VelocityStencil smoothness is missing"))


def test_python_refusals(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd import weno_vi
    from orthogonalsphericalshellgrids.jl_amd._operator_plan import OperatorPlan
    from orthogonalsphericalshellgrids.jl_amd.momentum import _MomentumTendencyPlan
    for name in ("weno_vi_momentum_advection_tendency", "weno_vi_momentum_advection_plan", "WenoViMomentumAdvectionPlan", "OnlySelfUpwinding"):
        assert hasattr(osg, name), name
    for name in ("weno_vi_lib", "check_weno_vi", "WENO_VI_SIGNATURES", "WENO_VI_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    assert issubclass(osg.WenoViMomentumAdvectionPlan, _MomentumTendencyPlan) and issubclass(osg.WenoViMomentumAdvectionPlan, OperatorPlan)
    assert osg.WenoViMomentumAdvectionPlan._HALO == (3, 3, 1)
    assert osg.WenoViMomentumAdvectionPlan._SPACINGS[1] is osg.z_center_spacings
    assert osg.WenoMomentumAdvectionPlan._SPACINGS[1] is osg.z_all_face_spacings is osg.MomentumAdvectionPlan._SPACINGS[1]
    grid, other = _grid(osg), _grid(osg)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))       # noqa: E731
    window = (slice(None), slice(None), range(1, 3))
    B = weno_vi.BUILT
    import dataclasses
    for fn in (osg.weno_vi_momentum_advection_plan, lambda u_, v_, w_, a, b, **kw: osg.weno_vi_momentum_advection_tendency(u_, v_, w_, out=(a, b), **kw)):
        # the schemes: checked first, each message names what is built
        with pytest.raises(NotImplementedError, match="enstrophy-conserving vorticity term is momentum_advection_plan's") as e:
            fn(u, v, w, Gu, Gv, scheme=osg.VectorInvariant())
        assert BUILT_NAME in str(e.value)
        with pytest.raises(NotImplementedError, match="centred vertical term and kinetic-energy gradient are weno_momentum_advection_plan's") as e:
            fn(u, v, w, Gu, Gv, scheme=osg.VectorInvariant(vorticity_scheme=osg.WENO(order=5)))
        assert BUILT_NAME in str(e.value)
        for field in ("vorticity_scheme", "vertical_scheme", "kinetic_energy_gradient_scheme", "divergence_scheme"):
            with pytest.raises(NotImplementedError, match="WENO of order 7 is not built") as e:
                fn(u, v, w, Gu, Gv, scheme=dataclasses.replace(B, **{field: osg.WENO(order=7)}))
            assert BUILT_NAME in str(e.value)
        with pytest.raises(NotImplementedError, match="WENO of order 3 is not built"):
            fn(u, v, w, Gu, Gv, scheme=dataclasses.replace(B, upwinding=osg.OnlySelfUpwinding(cross_scheme=osg.WENO(order=3))))
        with pytest.raises(NotImplementedError, match="VelocityStencil smoothness is not built") as e:
            fn(u, v, w, Gu, Gv, scheme=dataclasses.replace(B, vorticity_stencil=osg.VelocityStencil()))
        assert BUILT_NAME in str(e.value)
        for scheme in ("weno", "enstrophy_conserving", None, osg.WENO(order=5), dataclasses.replace(B, upwinding=osg.OnlySelfUpwinding()),
                       dataclasses.replace(B, upwinding=None), dataclasses.replace(B, vertical_scheme=osg.EnergyConserving()),
                       dataclasses.replace(B, divergence_scheme=osg.Centered()), dataclasses.replace(B, kinetic_energy_gradient_scheme=None)):
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
        with pytest.raises(TypeError, match=r"Gu must be a Field at \(Face, Center, Center\)"):
            fn(u, v, w, Gv, Gv)
        with pytest.raises(TypeError, match=r"Gv must be a Field at \(Center, Face, Center\)"):
            fn(u, v, w, Gu, osg.XFaceField(grid))
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
        osg.weno_vi_momentum_advection_tendency(v, v, w)


def test_missing_library_fails_loudly(osg, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the plan raises: it computes nothing some other way"""
    missing = str(tmp_path / os.path.basename(osg._lib.WENO_VI_LIB_PATH))
    monkeypatch.setattr(osg._lib, "_weno_vi", None)
    monkeypatch.setattr(osg._lib, "WENO_VI_LIB_PATH", missing)
    grid = _grid(osg)
    with pytest.raises(ImportError, match="only backend"):
        osg.weno_vi_momentum_advection_plan(osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid))


def test_the_build_names_the_library_the_map_and_the_shared_definitions():
    from test_abi import ROOT
    csrc = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    text = open(os.path.join(csrc, "weno_vi.map")).read()
    assert all(n in text for n in NAMES) and "local: *;" in text
    # W5F has one definition in the tree, beside weno_face; the kernel file includes it and the shared host layer and defines neither
    face = open(os.path.join(csrc, "tpg_weno_face.hpp")).read()
    assert face.count("T weno_face_fs(") == 1 and face.count("T weno_face(") == 1 and face.count("T weno_face3(") == 1
    body = open(os.path.join(csrc, "tpg_weno_vi.hip")).read()
    assert '#include "tpg_weno_face.hpp"' in body and '#include "tpg_momentum_tendency.hpp"' in body
    assert "T weno_face" not in body and "struct MomentumCall" not in body and "atomic" not in body.replace("No atomics", "").replace("no atomics", "")
    # the WENO5 vorticity kernel has one definition, a header both momentum files include; the pointer struct and the Args have one too
    kernel = "tpg_weno_vorticity_kernel.hpp"
    assert kernel in [ln for ln in make.split("\n") if ln.startswith("HDRS")][0].split()
    sources = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".hpp"))}
    assert all(f'#include "{kernel}"' in sources[n] for n in ("tpg_weno_momentum.hip", "tpg_weno_vi.hip"))
    assert [n for n, text in sources.items() if "auto zeta_at" in text] == [kernel] and sources[kernel].count("auto zeta_at") == 1
    assert "__shfl" not in body and "TPG_WMOM" not in body and "TPG_W" not in sources[kernel]
    for struct in ("struct MomentumPtrs", "struct MomentumArgs"):
        assert sum(text.count(struct) for text in sources.values()) == 1 and struct in sources["tpg_momentum_tendency.hpp"]
    assert not any(old in text for old in ("MomPtrs", "WmomPtrs", "WviPtrs") for text in sources.values())
    import json
    diff = json.load(open(os.path.join(ROOT, "profiles", "weno_vi", "isa_diff.json")))
    assert all(r.get("code_object_identical", True) for r in diff.values()) and "tpg_weno_momentum.o" in diff and "tpg_momentum.o" in diff
