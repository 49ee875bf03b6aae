// weno_vs_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_weno_vs_momentum_advection_tendency, for a
// sanitizer build of the HOST code of libtripolar_hip_weno_vs.so (tpg_weno_vs.hip over tpg_momentum_tendency.hpp: the Span tables, the
// overlap arithmetic) with the error channel, in the manner of tools/momentum_argcheck.cpp.  The seven refusals of the header, in its order.
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/weno_vs_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_weno_vs.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip \
//         -ldl -o weno_vs_argcheck
//   ./weno_vs_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_weno_vs.h"

static int failures = 0;

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Args {
    const void *u, *v, *w;
    void *Gu, *Gv;
    const void* m[9];                                              // dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_c
    const int32_t *nfc, *ncf;
    int Nx = 48, Ny = 40, Nz = 3, Hx = 4, Hy = 4, Hz = 4, ft = TPG_F64;
};

static void expect(const Args& a, int want, const char* starts, int line)
{
    const int rc = tpg_weno_vs_momentum_advection_tendency(a.u, a.v, a.w, a.Gu, a.Gv, a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.m[6], a.m[7],
                                                           a.m[8], a.nfc, a.ncf, 0.1, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
    const char* msg = tpg_weno_vs_last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(args, want, starts) expect((args), (want), (starts), __LINE__)

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
    // 1. the geometry
    a = ok; a.ft = 7;            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    a = ok; a.Nx = 49;           EXPECT(a, TPG_ERR_ODD_NLAMBDA, "");
    a = ok; a.Nz = 0;            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "invalid size");
    // 2. null pointers, each group before what follows it
    a = ok; a.u = nullptr; a.Gu = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.v = nullptr;       EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.w = nullptr;       EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.Gv = nullptr; a.m[0] = nullptr; EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null Gu or Gv");
    for (int q = 0; q < 9; ++q) {
        a = ok; a.m[q] = nullptr;
        EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_c");
    }
    // 3. one count plane without the other
    a = ok; a.ncf = nullptr;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_cf is null)");
    a = ok; a.nfc = nullptr;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_fc is null)");
    // 4. alignment
    a = ok; a.w = at(base + 2 * parent + 4);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "u, v or w pointer not aligned");
    a = ok; a.Gu = at(far + 2); a.ft = TPG_F32; EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu or Gv pointer not aligned");
    for (int q = 0; q < 9; ++q) {
        a = ok; a.m[q] = at(((uintptr_t)(q + 1) << 20) + 4);
        EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_c pointer not aligned");
    }
    a = ok; a.ncf = static_cast<const int32_t*>(at((21 << 20) + 2)); EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    // 5. the overlaps
    a = ok; a.Gu = const_cast<void*>(ok.v);            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu overlaps v");
    a = ok; a.Gv = at(base + 8);                       EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps u");
    a = ok; a.Gv = at(far + parent - 8);               EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps Gu");
    a = ok; a.Gv = at(base + 2 * parent + wparent - 8); EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps w");   // the last element of w's longer parent
    a = ok; a.Gv = at(base + 2 * parent + wparent); a.Hz = 0;                 // right behind it: no overlap, the call goes on to the halo check
    EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    // 6. the halo of the stencil
    a = ok; a.Hx = 2; a.nfc = a.ncf = nullptr;
    EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads u, v[i-3..i+3, j-3..j+3, k-3..k+3 within 0..Nz+1] and w[i-2..i+1, j], w[i, j-2..j+1]: "
                                   "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,4,4))");
    a = ok; a.Hy = 2;            EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hx = 3; a.Hy = 3; a.Hz = 1; a.Gu = nullptr;   EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null Gu or Gv");   // the minimum halo is not refused for its halo
    // 7. too large for 32-bit indexing: refused by the plane check every entry point shares
    Args big = ok;
    big.u = at(1ull << 44); big.v = at(2ull << 44); big.w = at(3ull << 44); big.Gu = at(4ull << 44); big.Gv = at(5ull << 44);
    big.nfc = big.ncf = nullptr; big.Nx = 65536; big.Ny = 32768; big.Nz = 1; big.Hx = big.Hy = 3; big.Hz = 1; big.ft = TPG_F32;
    EXPECT(big, TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("weno_vs_argcheck: every call refused in validation, as expected");
    return 0;
}
