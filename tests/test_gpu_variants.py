"""Every kernel variant kept in the library (the simple thread-per-cell build kernel and the LDS-tile default; the
zipper's row-item and column-item forms) must produce identical bits: they differ only in how the same arithmetic is
scheduled.  The TPG_* knobs exist in the TEST library only (tools/libtripolar_hip_test.so; the product library reads no
environment variable): they are read once into an immutable record; tpg_reload_config() publishes a new one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
KNOBS = ("TPG_CELLS_VARIANT", "TPG_BUILD_NT", "TPG_ZIPPER_VARIANT")


@pytest.fixture
def knob(osg, via_testlib):
    saved = {k: os.environ.get(k) for k in KNOBS}
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    via_testlib.tpg_reload_config()


@pytest.mark.parametrize("kw", [dict(size=(250, 100, 1)),
                                dict(size=(128, 64, 1), halo=(3, 2, 1), north_poles_latitude=65),
                                dict(size=(64, 20, 1), dtype=torch.float32),
                                dict(size=(360, 180, 1), halo=(5, 5, 5)),                           # the reference's model halo
                                dict(size=(60, 10, 1)),                                             # Ny = 2 Hy + 2: k_south runs as a launch of its own
                                dict(size=(8, 40, 1), halo=(4, 2, 1))],                             # Nx < 2 Hx + 2: narrower than its two x halos
                         ids=["250x100", "128x64", "64x20-f32", "360x180-halo5", "60x10-short", "8x40-narrow"])
def test_build_kernel_variants_agree(osg, gpu, knob, kw):
    kw = dict(kw)
    dtype = kw.pop("dtype", torch.float64)
    results = {}
    for variant, nt in ((0, 1), (0, 0), (2, 1), (2, 0)):     # 0: thread per cell; 2: LDS tile kernel (the product's form)
        knob["TPG_CELLS_VARIANT"], knob["TPG_BUILD_NT"] = str(variant), str(nt)
        osg._lib.lib().tpg_reload_config()
        g = osg.TripolarGrid(osg.GPU(0), dtype, **kw)
        results[(variant, nt)] = {n: getattr(g, n).cpu().numpy() for n in osg._lib.ARRAY_NAMES}
    ref = results[(0, 1)]
    for key, arrs in results.items():
        for n, a in arrs.items():
            assert np.array_equal(a, ref[n], equal_nan=True), (key, n)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_zipper_kernel_variants_agree(osg, gpu, knob, dtype):
    size, halo = (256, 40, 4), (4, 4, 2)
    grid = osg.TripolarGrid(osg.GPU(0), dtype, size=size, halo=halo)
    rng = np.random.default_rng(4)
    specs = [(xl, yl, sg) for xl in (0, 1) for yl in (0, 1) for sg in (1, -1)]
    hosts = [rng.uniform(-1, 1, (4 + 4, 40 + 8, 256 + 8)).astype(np.float64 if dtype == torch.float64 else np.float32) for _ in specs]
    outs = {}
    for variant in (0, 3):
        knob["TPG_ZIPPER_VARIANT"] = str(variant)
        osg._lib.lib().tpg_reload_config()
        fs = []
        for (xl, yl, sg), h in zip(specs, hosts):
            loc = (osg.Face if xl else osg.Center, osg.Face if yl else osg.Center, osg.Center)
            f = osg.Field(loc, grid, boundary_conditions=osg.FieldBoundaryConditions(north=osg.ZipperBoundaryCondition(sg)))
            f.data.copy_(torch.from_numpy(h))
            fs.append(f)
        osg.fill_halo_regions(fs)
        outs[variant] = [f.data.cpu().numpy() for f in fs]
    for variant, arrs in outs.items():
        for a, b in zip(arrs, outs[0]):
            assert np.array_equal(a, b), variant


def test_knobs_are_read_once(osg, gpu, knob):
    """an environment change without tpg_reload_config() must not flip kernels between calls (getenv per call)"""
    lib = osg._lib.lib()
    knob["TPG_ZIPPER_VARIANT"] = "3"
    lib.tpg_reload_config()
    knob["TPG_ZIPPER_VARIANT"] = "0"                  # not reloaded: still the column kernel ...
    d = torch.zeros((1 + 2, 8 + 8, 16 + 8), dtype=torch.float64, device=gpu)
    import ctypes as C
    # ... which the copy probe requires (it refuses geometries without a column kernel, not the knob)
    assert lib.tpg_zipper_copy_probe(osg._lib.ptr_table([d]), 1, (C.c_int8 * 1)(0), 16, 8, 1, 4, 4, 1, 1, None, None, None) == 0
    torch.cuda.synchronize()


def test_product_library_ignores_the_knobs(osg, gpu):
    """libtripolar_hip.so reads no environment variable: with TPG_FILL_MERGED=0 / TPG_ZIPPER_VARIANT=0 exported it still exports no
    reload hook and produces the same fill (the default kernels)"""
    lib = osg._lib.lib()
    assert not hasattr(lib, "tpg_reload_config")
    saved = {k: os.environ.get(k) for k in ("TPG_ZIPPER_VARIANT", "TPG_FILL_MERGED", "TPG_FILL_FUSED")}
    try:
        grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=(64, 40, 2), halo=(4, 4, 2))
        u = osg.XFaceField(grid)
        u.data.copy_(torch.rand_like(u.data))
        a = u.data.clone()
        osg.fill_halo_regions([u])
        want = u.data.clone()
        os.environ.update(TPG_ZIPPER_VARIANT="0", TPG_FILL_MERGED="0", TPG_FILL_FUSED="0")
        u.data.copy_(a)
        osg.fill_halo_regions([u])
        assert torch.equal(u.data, want)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
