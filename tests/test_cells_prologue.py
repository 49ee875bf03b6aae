"""The prologue of k_cells_tile (csrc/tpg_grid.hip, csrc/tpg_tiles.hpp, tpgb::kAtanTable in csrc/tpg_batch.hpp;
profiles/cells_prologue/README.md): the loads of a wave's first round trips were reordered and the integer arithmetic in front of them lost
its divisions, so no bit of any of the 20 arrays may change.

CPU: csrc/tpg_tiles.hpp is compiled for the host and held against `/`, `%` and the functions it replaces --
  * divmod_rcp with the host's reciprocal against `/` and `%` for every tiles_x in 1 .. 1024: every t in 0 .. min(tiles, 2^20) and the last
    2^12 numbers below tiles, for the largest launch the host admits (tiles_y = 65535) and for tiles_y = 1, 2, 3, 257;
  * tile_xy(tile_of_block(b)) against the previous tile_of_block followed by `/` and `%`, for both values of `grouped`, over the same sets
    (a block id b runs over the same numbers as t);
  * wrap_col, whose test for the generic modulo became wave-uniform, against the per-lane form, for every Nx in 1 .. 1024 and every column
    any lane of any tile forms;
  * the atan table image against the table as it was built before: rows by row / column, LUT by word.
GPU: all 20 whole padded arrays of tpg_build_grid against the oracle and against the thread-per-cell kernel (TPG_CELLS_VARIANT=0 of the test
library) at Nx = 60 (one tile per row), 64 (the last tile has two columns), 124 x Ny = 15..21; 360 x 180 (6 x 26 = 156 tiles: two whole
groups of 64 block ids and a partial one) in both tile orders (TPG_CELLS_ORDER 0, 1); Float32 at Nx = 62; first-pole longitudes with
fplp90 = 45, 160.3, 190.7, 225 and 380 (above 360: every row takes the general path); latitude bands with jstart = 1 and 8, 15, 21.
3600 x 1800 is tests/test_gpu_grid.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_cells_trims3 import _HIP_STUB      # what the headers need of the HIP device environment, for a host compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orthogonalsphericalshellgrids.jl_amd", "csrc")

# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
_HARNESS = r"""
#include <initializer_list>
#include <thread>
#include "tpg_tiles.hpp"
#include "tpg_batch.hpp"

namespace previous {
int tile_of_block(int b, int tiles, bool grouped)
{
    const int base = b & ~63;
    if (grouped && base + 64 <= tiles) return base + (b & 7) * 8 + ((b >> 3) & 7);
    return b;
}
int wrap_col(int v, int Nx)
{
    if (v < 1) v += Nx;
    if (v > Nx) v -= Nx;
    if (v < 1 || v > Nx) { v = (v - 1) % Nx; v = (v < 0 ? v + Nx : v) + 1; }
    return v;
}
// the atan table as every wave built it: LUT words by thread, rows by thread / 6 and thread % 6
void atan_table_init(double* tab, int tid)
{
    static const unsigned lut[24] = {
        0x30303000u, 0x30303030u, 0x30303030u, 0x30303030u, 0x30303030u, 0x60606030u, 0x60606060u, 0x60606060u,
        0x60606060u, 0x60606060u, 0x60606060u, 0x90606060u, 0x90909090u, 0x90909090u, 0x90909090u, 0x90909090u,
        0x90909090u, 0x90909090u, 0x90909090u, 0x90909090u, 0xC0C0C0C0u, 0xC0C0C0C0u, 0xC0C0C0C0u, 0xC0C0C0C0u };
    if (tid < 24) reinterpret_cast<unsigned*>(tab + TPG_ATAN_ROWS_DOUBLES)[tid] = lut[tid];
    const double rows[5][6] = {
        { 1.0, 0.0, 1.0, 0.0, 0.0, 0.0 },
        { 2.0, 1.0, 2.0, 1.0, 0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56 },
        { 1.0, 1.0, 1.0, 1.0, 0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55 },
        { 1.0, 1.5, 1.0, 1.5, 0x1.f730bd281f69bp-1, 0x1.007887af0cbbdp-56 },
        { 0.0, 1.0, 0.0, 1.0, tpgm::kPio2Hi, tpgm::kPio2Lo } };
    if (tid < TPG_ATAN_ROWS_DOUBLES) tab[tid] = rows[tid / 6][tid % 6];
}
}  // namespace previous

namespace {
// one number t of a launch of tiles_x x tiles_y tiles: the division, and the tile of block id t in both orders.  bad[0..2]: the first failure
bool one(unsigned t, int tiles_x, int tiles_y, unsigned rcp, long long* bad)
{
    const int tiles = tiles_x * tiles_y;
    const tpgt::DivMod dm = tpgt::divmod_rcp(t, (unsigned)tiles_x, rcp);
    bool ok = dm.q == t / (unsigned)tiles_x && dm.r == t % (unsigned)tiles_x;
    if (t < (unsigned)tiles) {
        for (int grouped = 0; grouped < 2; ++grouped) {
            const int tn = tpgt::tile_of_block((int)t, tiles, grouped != 0), tp = previous::tile_of_block((int)t, tiles, grouped != 0);
            const tpgt::TileXY xy = tpgt::tile_xy(tn, tiles_x, tiles_y, rcp);
            ok = ok && tn == tp && tn >= 0 && tn < tiles && xy.ty == tiles_y - 1 - tp / tiles_x && xy.tx == tp % tiles_x;
        }
    }
    if (!ok && bad[0] < 0) { bad[0] = t; bad[1] = tiles_x; bad[2] = tiles_y; }
    return ok;
}
}  // namespace

extern "C" {
// every tiles_x in lo .. hi with tiles_y: t in 0 .. min(tiles, 2^20) and the last 2^12 numbers up to tiles; returns the number of failures
// (four threads, tiles_x dealt round-robin: 10^9 numbers with four hardware divisions each)
long long check_tiles(int lo, int hi, int tiles_y, long long* bad, long long* checked)
{
    enum { NT = 4 };
    long long fails[NT] = {}, n[NT] = {}, first[NT][3];
    std::thread th[NT];
    for (int w = 0; w < NT; ++w) {
        first[w][0] = -1;
        th[w] = std::thread([=, &fails, &n, &first] {
            long long f = 0, c = 0;
            for (int tiles_x = lo + w; tiles_x <= hi; tiles_x += NT) {
                const unsigned rcp = tpgt::rcp_of((unsigned)tiles_x);
                const long long tiles = (long long)tiles_x * tiles_y, head = tiles < (1ll << 20) ? tiles : (1ll << 20);
                for (long long t = 0; t <= head; ++t, ++c) f += !one((unsigned)t, tiles_x, tiles_y, rcp, first[w]);
                for (long long t = tiles - 4096 > head ? tiles - 4096 : head + 1; t <= tiles; ++t, ++c) f += !one((unsigned)t, tiles_x, tiles_y, rcp, first[w]);
            }
            fails[w] = f; n[w] = c;
        });
    }
    long long total = 0;
    *checked = 0; bad[0] = -1;
    for (int w = 0; w < NT; ++w) {
        th[w].join();
        total += fails[w]; *checked += n[w];
        if (first[w][0] >= 0 && bad[0] < 0) { bad[0] = first[w][0]; bad[1] = first[w][1]; bad[2] = first[w][2]; }
    }
    return total;
}
// the division alone at the ends of the 32-bit range, any d in lo .. hi
long long check_divmod_ends(unsigned lo, unsigned hi)
{
    long long fails = 0;
    for (unsigned d = lo; d <= hi; ++d) {
        const unsigned rcp = tpgt::rcp_of(d);
        for (unsigned k = 0; k < 4096; ++k)
            for (unsigned t : { k, 0x7FFFFFFFu - k, 0x80000000u + k, 0xFFFFFFFFu - k, d * k, d * k + d - 1u }) {
                const tpgt::DivMod dm = tpgt::divmod_rcp(t, d, rcp);
                fails += !(dm.q == t / d && dm.r == t % d);
            }
    }
    return fails;
}
// every column any lane of any tile of a grid of Nx columns forms (k_cells_tile: shift = Nx / 4, tiles_x = ceil((Nx / 2) / 30), hl = 0 .. 31)
long long check_wrap(int lo, int hi, long long* checked)
{
    long long fails = 0, n = 0;
    for (int Nx = lo; Nx <= hi; ++Nx) {
        const int shift = Nx / 4, tiles_x = (Nx / 2 + 29) / 30;
        for (int tx = 0; tx < tiles_x; ++tx)
            for (int hl = 0; hl < 32; ++hl)
                for (int v : { shift + 30 * tx + hl, shift - 30 * tx - 30 + hl }) {
                    const int w = tpgt::wrap_col(v, Nx);
                    fails += !(w == previous::wrap_col(v, Nx) && w >= 1 && w <= Nx);
                    ++n;
                }
    }
    *checked = n;
    return fails;
}
// the table from the image, copied by `threads` threads, and the table of before by 64
void atan_tables(int threads, double* now, double* before)
{
    for (int t = 0; t < threads; ++t) tpgb::atan_table_init(now, t);
    for (int t = 0; t < 64; ++t) previous::atan_table_init(before, t);
}
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/tpg_tiles.hpp and the atan table of csrc/tpg_batch.hpp compiled for the host, beside the forms they replace"""
    d = tmp_path_factory.mktemp("prologue")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text(_HIP_STUB)
    (d / "harness.cpp").write_text(_HARNESS)
    so = d / "libprologue.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-pthread", "-Wno-unknown-pragmas",
                        "-Wno-attributes", "-I", str(d), "-I", CSRC, "-o", str(so), str(d / "harness.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(str(so))
    ll = C.POINTER(C.c_longlong)
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.check_tiles.argtypes, lib.check_tiles.restype = [C.c_int, C.c_int, C.c_int, ll, ll], C.c_longlong
    lib.check_divmod_ends.argtypes, lib.check_divmod_ends.restype = [C.c_uint, C.c_uint], C.c_longlong
    lib.check_wrap.argtypes, lib.check_wrap.restype = [C.c_int, C.c_int, ll], C.c_longlong
    lib.atan_tables.argtypes, lib.atan_tables.restype = [C.c_int, dp, dp], None
    return lib


@pytest.mark.parametrize("tiles_y", [65535, 1, 2, 3, 257])
def test_reciprocal_division_and_tile_order_equal_the_divisions(host, tiles_y):
    """tiles_y = 65535 is the largest the launch admits: tiles = tiles_x tiles_y up to 1024 x 65535 < 2^26"""
    bad, n = (C.c_longlong * 3)(), C.c_longlong()
    fails = host.check_tiles(1, 1024, tiles_y, bad, C.byref(n))
    assert fails == 0, (fails, "first: t, tiles_x, tiles_y =", list(bad))
    assert n.value >= (1000 * 2 ** 20 if tiles_y == 65535 else 1024 * 1025 // 2 * tiles_y)


def test_reciprocal_division_holds_over_the_whole_32_bit_range(host):
    assert host.check_divmod_ends(1, 4096) == 0
    assert host.check_divmod_ends(2 ** 31 - 64, 2 ** 31 - 1) == 0            # d < 2^31 is the sign step's domain


def test_wave_uniform_wrap_equals_the_per_lane_wrap(host):
    n = C.c_longlong()
    assert host.check_wrap(1, 1024, C.byref(n)) == 0
    assert n.value > 64 * 1024


@pytest.mark.parametrize("threads", [64, 256, 42])
def test_atan_table_image_is_the_table_of_before(host, threads):
    now, before = np.full(42, np.nan), np.full(42, np.nan)
    host.atan_tables(threads, now, before)
    assert np.array_equal(now.view(np.uint64), before.view(np.uint64))


# ---- GPU: whole padded arrays ------------------------------------------------------------------------------------------------------
H4 = (4, 4, 4)
# (size, extra keywords, float32?, (ranks, rank) of a latitude band or None, TPG_CELLS_ORDER or None = the product's)
CASES = [((nx, ny, 1), {}, False, None, None) for nx in (60, 64, 124) for ny in range(15, 22)]
CASES += [((360, 180, 1), {}, False, None, order) for order in (0, 1)]           # 156 tiles: the order matters from 64 tiles on
CASES += [((124, 21, 1), {}, False, None, 0)]
CASES += [((62, 18, 1), {}, True, None, None)]                                   # Float32, Nx = 2 (mod 4)
# fplp90 = 45, 160.3, 190.7, 225 | 380: beyond 360 the whole grid takes the general path
CASES += [((124, 20, 1), dict(first_pole_longitude=fpl), False, None, None) for fpl in (-45.0, 70.3, 100.7, 135.0, 290.0)]
# bands of 7 rows of a 124 x 21 grid: jstart = 1 (the apron row of the lowest tile row is row 0), 8, 15; of 60 x 40 in two: jstart = 1, 21
CASES += [((124, 21, 1), {}, False, (3, r), None) for r in range(3)] + [((60, 40, 1), {}, False, (2, r), None) for r in range(2)]


def _id(case):
    size, kw, f32, band, order = case
    return (f"{size[0]}x{size[1]}" + ("-f32" if f32 else "") + (f"-fpl{kw['first_pole_longitude']}" if kw else "")
            + (f"-band{band[1]}of{band[0]}" if band else "") + ("" if order is None else f"-order{order}"))


_ref = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _arrays(osg, case):
    import torch
    size, kw, f32, band, _ = case
    arch = osg.GPU(0) if band is None else osg.Distributed(osg.GPU(0), osg.Partition(y=band[0]), local_rank=band[1])
    g = osg.TripolarGrid(arch, torch.float32 if f32 else torch.float64, size=size, halo=H4, **kw)
    return {n: getattr(g, n).cpu().numpy() for n in osg._lib.ARRAY_NAMES}, (g.jrange if band else None)


def _reference(oracle, case, jrange):
    """the oracle's arrays of a case: computed once, shared by the tile orders, left unchanged"""
    size, kw, f32, band, _ = case
    key = _id(case[:4] + (None,))
    if key not in _ref:
        rows = {} if jrange is None else dict(jstart=jrange[0], jend=jrange[1])
        ref = oracle.build_grid(size, dtype=np.float32 if f32 else np.float64, halo=H4, **kw, **rows)
        for a in ref.values():
            a.setflags(write=False)
        _ref[key] = ref
    return _ref[key]


def _assert_same(got, want, what):
    assert len(want) == 20 and set(got) == set(want)
    for name, r in want.items():
        a = got[name]
        assert a.shape == r.shape and a.dtype == r.dtype, (what, name)
        same = _bits(a) == _bits(r)
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def test_cases_cover_what_the_prologue_can_get_wrong():
    sizes = {c[0][:2] for c in CASES}
    assert {(nx, ny) for nx in (60, 64, 124) for ny in range(15, 22)} <= sizes and (360, 180) in sizes
    assert {c[4] for c in CASES if c[0][:2] == (360, 180)} == {0, 1}
    assert (360 // 2 + 29) // 30 * ((180 + 6) // 7) == 156                       # 360 x 180: jm_lo .. jm_hi = 1 .. 180, 7 cell rows per tile
    assert any(c[2] and c[0][0] == 62 for c in CASES)
    assert {c[1]["first_pole_longitude"] + 90.0 for c in CASES if c[1]} == {45.0, 160.3, 190.7, 225.0, 380.0}
    starts = {c[3][1] * (c[0][1] // c[3][0]) + 1 for c in CASES if c[3]}
    assert starts == {1, 8, 15, 21}


@pytest.fixture
def knobs(osg, via_testlib):
    """TPG_CELLS_VARIANT / TPG_CELLS_ORDER of the test library, restored afterwards"""
    names = ("TPG_CELLS_VARIANT", "TPG_CELLS_ORDER")
    saved = {n: os.environ.get(n) for n in names}

    def select(**kw):
        for n in names:
            v = kw.get(n)
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = str(v)
        via_testlib.tpg_reload_config()
    yield select
    for n, v in saved.items():
        if v is None:
            os.environ.pop(n, None)
        else:
            os.environ[n] = v
    via_testlib.tpg_reload_config()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_all_twenty_arrays_equal_the_oracle_bit_for_bit(osg, oracle, gpu, knobs, case):
    knobs(TPG_CELLS_VARIANT=2, TPG_CELLS_ORDER=case[4])
    got, jrange = _arrays(osg, case)
    if case[3]:
        ny = case[0][1] // case[3][0]
        assert tuple(jrange) == (case[3][1] * ny + 1, case[3][1] * ny + ny)
    _assert_same(got, _reference(oracle, case, jrange), "oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_tile_kernel_equals_the_thread_per_cell_kernel(osg, gpu, knobs, case):
    knobs(TPG_CELLS_VARIANT=0)
    want, _ = _arrays(osg, case)
    knobs(TPG_CELLS_VARIANT=2, TPG_CELLS_ORDER=case[4])
    got, _ = _arrays(osg, case)
    _assert_same(got, want, "thread per cell")
