"""Host-side tests of the momentum advection tendency of the drivers' WENOVectorInvariant(vorticity_order = 5) (no GPU): the export list of
libtripolar_hip_weno_vs.so, every argument error of tpg_weno_vs_momentum_advection_tendency in the order the header gives (status and
message; every call below fails in validation, none reaches a launch, the pointers are fabricated and never dereferenced), every refusal of
the Python layer on host-only grid records, the record, the refusals of the older calls that must stay as they are, the loader, and the
names the build is made of."""
import dataclasses
import os

import pytest

from test_weno_momentum_conditions import BASE, FAR, G, GU, GV, NCF, NFC, PARENT, PLANE, U, V, W, WPARENT, _grid
from test_weno_vi_conditions import AT, METRICS, NULL_METRIC, OFF_METRIC, STENCIL

NAMES = ["tpg_weno_vs_last_error", "tpg_weno_vs_momentum_advection_tendency"]
BUILT_NAME = ("VectorInvariant(vorticity_scheme=WENO(order=5), vorticity_stencil=VelocityStencil(), vertical_scheme=WENO(order=5), "
              "kinetic_energy_gradient_scheme=WENO(order=5), divergence_scheme=WENO(order=5), "
              "upwinding=OnlySelfUpwinding(cross_scheme=WENO(order=5)))")


def _call(lib, n_fc=None, n_cf=None, geom=G, ft=1, **over):
    s = dict(u=U, v=V, w=W, Gu=GU, Gv=GV, **AT)
    s.update(over)
    return lib.tpg_weno_vs_momentum_advection_tendency(s["u"], s["v"], s["w"], s["Gu"], s["Gv"], *(s[k] for k in METRICS), n_fc, n_cf, 0.0,
                                                       *geom, ft, None)


def test_header_exports_and_signatures_are_the_two_names(osg):
    from test_abi import ROOT, declared_symbols, exported_symbols
    L = osg._lib
    L.weno_vs_lib()
    assert sorted(declared_symbols("tripolar_hip_weno_vs.h")) == NAMES == sorted(exported_symbols(L.WENO_VS_LIB_PATH)) == sorted(L.WENO_VS_SIGNATURES)
    # the signature is tpg_weno_vi_momentum_advection_tendency's, argument for argument
    assert L.WENO_VS_SIGNATURES["tpg_weno_vs_momentum_advection_tendency"] == L.WENO_VI_SIGNATURES["tpg_weno_vi_momentum_advection_tendency"]


def test_argument_errors_without_device_work(osg):
    """the seven refusals of tpg_weno_vi_momentum_advection_tendency, in that order, with its messages"""
    lib = osg._lib.weno_vs_lib()
    err = lambda: lib.tpg_weno_vs_last_error().decode()           # noqa: E731
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
    # and the same status and message as the call whose refusals these are, on one bad call of each kind
    vi = osg._lib.weno_vi_lib()
    for over in (dict(ft=7), dict(u=None), dict(Gv=None), dict(dz_c=None), dict(n_fc=NFC), dict(w=W + 4), dict(Gu=U), dict(geom=(48, 40, 3, 2, 4, 4))):
        s = dict(u=U, v=V, w=W, Gu=GU, Gv=GV, **AT)
        s.update({k: x for k, x in over.items() if k in s})
        args = (s["u"], s["v"], s["w"], s["Gu"], s["Gv"], *(s[k] for k in METRICS), over.get("n_fc"), None, 0.0, *over.get("geom", G), over.get("ft", 1), None)
        assert lib.tpg_weno_vs_momentum_advection_tendency(*args) == vi.tpg_weno_vi_momentum_advection_tendency(*args) < 0, over
        assert err() == vi.tpg_weno_vi_last_error().decode() != "", over


def test_the_record(osg):
    from orthogonalsphericalshellgrids.jl_amd import weno_momentum, weno_vi, weno_vs
    assert weno_vs.BUILT == dataclasses.replace(weno_vi.BUILT, vorticity_stencil=osg.VelocityStencil())
    assert weno_vs.BUILT == osg.VectorInvariant(vorticity_scheme=osg.WENO(order=5), vorticity_stencil=osg.VelocityStencil(),
                                                vertical_scheme=osg.WENO(order=5), kinetic_energy_gradient_scheme=osg.WENO(order=5),
                                                divergence_scheme=osg.WENO(order=5),
                                                upwinding=osg.OnlySelfUpwinding(cross_scheme=osg.WENO(order=5)))
    assert weno_vs.BUILT != weno_vi.BUILT != weno_momentum.BUILT and hash(weno_vs.BUILT) == hash(weno_vs.BUILT)
    assert weno_vs._BUILT_NAME == BUILT_NAME
    # the older records are what they were
    assert isinstance(weno_vi.BUILT.vorticity_stencil, osg.DefaultStencil) and isinstance(weno_momentum.BUILT.vorticity_stencil, osg.DefaultStencil)


def test_the_older_calls_still_refuse_velocity_stencil(osg):
    """once more, in one place: the two older plans and one-shot calls refuse a scheme with VelocityStencil(), this module's record among
    them, with their message; the drivers' constructor still raises"""
    from orthogonalsphericalshellgrids.jl_amd import weno_momentum, weno_vi, weno_vs
    grid = _grid(osg)
    f = lambda: (osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid))      # noqa: E731
    tendency = lambda fn: (lambda u, v, w, a, b, **kw: fn(u, v, w, out=(a, b), **kw))                                             # noqa: E731
    for fn, record in ((osg.weno_vi_momentum_advection_plan, weno_vi.BUILT), (tendency(osg.weno_vi_momentum_advection_tendency), weno_vi.BUILT),
                       (osg.weno_momentum_advection_plan, weno_momentum.BUILT), (tendency(osg.weno_momentum_advection_tendency), weno_momentum.BUILT)):
        for scheme in (weno_vs.BUILT, dataclasses.replace(record, vorticity_stencil=osg.VelocityStencil())):
            with pytest.raises(NotImplementedError, match="VelocityStencil smoothness is not built"):
                fn(*f(), scheme=scheme)
    with pytest.raises(NotImplementedError, match="is not built"):
        osg.momentum_advection_plan(*f(), scheme=weno_vs.BUILT)
    with pytest.raises(NotImplementedError, match="VelocityStencil smoothness is missing"):
        osg.WENOVectorInvariant(vorticity_order=5)


def test_python_refusals(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd import weno_momentum, weno_vi, weno_vs
    from orthogonalsphericalshellgrids.jl_amd._operator_plan import OperatorPlan
    from orthogonalsphericalshellgrids.jl_amd.momentum import _MomentumTendencyPlan
    for name in ("weno_vs_momentum_advection_tendency", "weno_vs_momentum_advection_plan", "WenoVsMomentumAdvectionPlan"):
        assert hasattr(osg, name), name
    for name in ("weno_vs_lib", "check_weno_vs", "WENO_VS_SIGNATURES", "WENO_VS_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    assert issubclass(osg.WenoVsMomentumAdvectionPlan, _MomentumTendencyPlan) and issubclass(osg.WenoVsMomentumAdvectionPlan, OperatorPlan)
    assert osg.WenoVsMomentumAdvectionPlan._HALO == (3, 3, 1)
    assert osg.WenoVsMomentumAdvectionPlan._SPACINGS[1] is osg.z_center_spacings
    assert osg.WenoVsMomentumAdvectionPlan._LIBRARY == ("weno_vs_lib", "check_weno_vs", "tpg_weno_vs_momentum_advection_tendency")
    grid, other = _grid(osg), _grid(osg)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))       # noqa: E731
    window = (slice(None), slice(None), range(1, 3))
    B = weno_vs.BUILT
    for fn in (osg.weno_vs_momentum_advection_plan, lambda u_, v_, w_, a, b, **kw: osg.weno_vs_momentum_advection_tendency(u_, v_, w_, out=(a, b), **kw)):
        # the schemes: checked first, each message names what is built where
        with pytest.raises(NotImplementedError, match="enstrophy-conserving vorticity term is momentum_advection_plan's") as e:
            fn(u, v, w, Gu, Gv, scheme=osg.VectorInvariant())
        assert BUILT_NAME in str(e.value)
        for scheme in (weno_vi.BUILT, weno_momentum.BUILT):
            with pytest.raises(NotImplementedError, match="DefaultStencil smoothness is weno_vi_momentum_advection_plan's") as e:
                fn(u, v, w, Gu, Gv, scheme=scheme)
            assert BUILT_NAME in str(e.value) and "weno_momentum_advection_plan" in str(e.value)
        for field in ("vorticity_scheme", "vertical_scheme", "kinetic_energy_gradient_scheme", "divergence_scheme"):
            with pytest.raises(NotImplementedError, match="WENO of order 7 is not built") as e:
                fn(u, v, w, Gu, Gv, scheme=dataclasses.replace(B, **{field: osg.WENO(order=7)}))
            assert BUILT_NAME in str(e.value)
        with pytest.raises(NotImplementedError, match="WENO of order 3 is not built"):
            fn(u, v, w, Gu, Gv, scheme=dataclasses.replace(B, upwinding=osg.OnlySelfUpwinding(cross_scheme=osg.WENO(order=3))))
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
        osg.weno_vs_momentum_advection_tendency(v, v, w)


def test_missing_library_fails_loudly(osg, monkeypatch, tmp_path):
    """no silent fallback: without its shared library the plan raises: it computes nothing some other way"""
    missing = str(tmp_path / os.path.basename(osg._lib.WENO_VS_LIB_PATH))
    monkeypatch.setattr(osg._lib, "_weno_vs", None)
    monkeypatch.setattr(osg._lib, "WENO_VS_LIB_PATH", missing)
    grid = _grid(osg)
    with pytest.raises(ImportError, match="only backend"):
        osg.weno_vs_momentum_advection_plan(osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid), osg.XFaceField(grid), osg.YFaceField(grid))


def test_the_build_names_the_library_the_map_and_the_shared_definitions():
    from test_abi import ROOT
    import json
    csrc = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    text = open(os.path.join(csrc, "weno_vs.map")).read()
    assert all(n in text for n in NAMES) and "local: *;" in text
    # W5V has one definition in the tree, beside the other face values; UB, VB at a chunk's edge have one, beside zeta_at
    sources = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".hpp"))}
    assert [n for n, t in sources.items() if "T weno_face_vs(" in t] == ["tpg_weno_face.hpp"] and sources["tpg_weno_face.hpp"].count("T weno_face_vs(") == 1
    kernel, finish = "tpg_weno_vorticity_kernel.hpp", "tpg_weno_vi_finish_kernel.hpp"
    for helper in ("auto ub_at", "auto vb_at"):
        assert [n for n, t in sources.items() if helper in t] == [kernel] and sources[kernel].count(helper) == 1
    # the finishing kernel has one definition, a header both translation units include; the new file defines no kernel of its own
    hdrs = [ln for ln in make.split("\n") if ln.startswith("HDRS")][0].split()
    assert kernel in hdrs and finish in hdrs
    assert [n for n, t in sources.items() if "void k_weno_vi_finish(" in t] == [finish]
    body = sources["tpg_weno_vs.hip"]
    assert all(f'#include "{h}"' in sources[n] for n in ("tpg_weno_vi.hip", "tpg_weno_vs.hip") for h in (kernel, finish))
    assert "__global__" not in body and "__shfl" not in body and "struct MomentumCall" not in body and "T weno_face" not in body
    assert "VS = true" in body and sources["tpg_weno_vi.hip"].count("VS = false") == 1 == sources["tpg_weno_momentum.hip"].count("VS = false")
    assert ", false>;" in body and ", true>;" not in body                                                 # the FULL form with this stencil is not built
    # the record of the build: nothing differs in an existing object, no scratch, no LDS, no spill in a committed instantiation
    diff = json.load(open(os.path.join(ROOT, "profiles", "weno_vs", "isa_diff.json")))
    assert "tpg_weno_momentum.o" in diff and "tpg_weno_vi.o" in diff and len(diff) >= 24
    for name, r in diff.items():
        assert not any(r.get(k) for k in ("differing", "metadata_differing", "only_old", "only_new")), name
    res = json.load(open(os.path.join(ROOT, "profiles", "weno_vs", "resources.json")))["kernels"]
    assert len(res) == 15 and sum("k_weno_momentum_advection" in k for k in res) == 5
    for k, r in res.items():
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"], r["group_segment_fixed_size"]) == ("0", "0", "0", "0"), k
        assert int(r["vgpr_count"]) <= 512, k
