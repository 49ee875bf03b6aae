// weno_momentum_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_weno_momentum_advection_tendency, for a sanitizer
// build of the HOST code of tpg_weno_momentum.hip (the Span tables, the overlap arithmetic, the error channel).
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/weno_momentum_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_weno_momentum.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o weno_momentum_argcheck
//   ./weno_momentum_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_weno_momentum.h"

static int failures = 0;

static void expect(int rc, int want, const char* starts, int line)
{
    const char* msg = tpg_weno_momentum_last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(call, want, starts) expect((call), (want), (starts), __LINE__)

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Args {
    const void *u, *v, *w;
    void *Gu, *Gv;
    const void* m[9];                                              // dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_f
    const int32_t *nfc, *ncf;
    int Nx = 48, Hx = 4, Hy = 4, Hz = 4, ft = TPG_F64;
};

static int call(const Args& a)
{
    return tpg_weno_momentum_advection_tendency(a.u, a.v, a.w, a.Gu, a.Gv, a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.m[6], a.m[7], a.m[8], a.nfc,
                                                a.ncf, 0.1, a.Nx, 40, 3, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

int main()
{
    const uintptr_t parent = 56ull * 48 * 11 * 8, wparent = 56ull * 48 * 12 * 8, base = 1ull << 30, far = 1ull << 40;
    Args ok;
    ok.u = at(base); ok.v = at(base + parent); ok.w = at(base + 2 * parent);
    ok.Gu = at(far); ok.Gv = at(far + 3 * parent);
    for (int q = 0; q < 9; ++q) ok.m[q] = at((uintptr_t)(q + 1) << 20);
    ok.nfc = static_cast<const int32_t*>(at(20 << 20));
    ok.ncf = static_cast<const int32_t*>(at(21 << 20));
    Args a;
    a = ok; a.ft = 7;            EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    a = ok; a.Nx = 49;           EXPECT(call(a), TPG_ERR_ODD_NLAMBDA, "");
    a = ok; a.v = nullptr;       EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.w = nullptr;       EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.Gv = nullptr;      EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null Gu or Gv");
    for (int q = 0; q < 9; ++q) {
        a = ok; a.m[q] = nullptr; EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f");
        a = ok; a.m[q] = at(((uintptr_t)(q + 1) << 20) + 4);
        EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f pointer not aligned");
    }
    a = ok; a.ncf = nullptr;     EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_cf is null)");
    a = ok; a.nfc = nullptr;     EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_fc is null)");
    a = ok; a.w = at(base + 2 * parent + 4);  EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "u, v or w pointer not aligned");
    a = ok; a.Gu = at(far + 2); a.ft = TPG_F32; EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "Gu or Gv pointer not aligned");
    a = ok; a.ncf = static_cast<const int32_t*>(at((21 << 20) + 2)); EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    a = ok; a.Gu = const_cast<void*>(ok.v);            EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "Gu overlaps v");
    a = ok; a.Gv = at(base + 8);                       EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "Gv overlaps u");
    a = ok; a.Gv = at(far + parent - 8);               EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "Gv overlaps Gu");
    a = ok; a.Gv = at(base + 2 * parent + wparent - 8); EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "Gv overlaps w");   // the last element of w's longer parent
    a = ok; a.Gv = at(base + 2 * parent + wparent); a.Hz = 0;                 // right behind it: no overlap, the call goes on to the halo check
    EXPECT(call(a), TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hx = 2; a.nfc = a.ncf = nullptr;         EXPECT(call(a), TPG_ERR_UNSUPPORTED, "the rule reads Z[i, j-2..j+3] and Z[i-2..i+3, j]");
    a = ok; a.Hy = 2;                                  EXPECT(call(a), TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hx = 3; a.Hy = 3; a.Hz = 1; a.Gu = nullptr;   EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null Gu or Gv");   // the minimum halo is not refused for its halo
    EXPECT(tpg_weno_momentum_advection_tendency(at(1ull << 44), at(2ull << 44), at(3ull << 44), at(4ull << 44), at(5ull << 44), ok.m[0], ok.m[1], ok.m[2], ok.m[3],
                                                ok.m[4], ok.m[5], ok.m[6], ok.m[7], ok.m[8], nullptr, nullptr, 0.0, 65536, 32768, 1, 3, 3, 1, TPG_F32, nullptr),
           TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("weno_momentum_argcheck: every call refused in validation, as expected");
    return 0;
}
