// momentum_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_momentum_advection_tendency,
// tpg_weno_momentum_advection_tendency and tpg_weno_vi_momentum_advection_tendency, for a sanitizer build of the HOST code the three share
// (tpg_momentum_tendency.hpp: the Span tables, the overlap arithmetic) with the error channel.  One table of bad calls goes through all
// three entry points (the third names its spacing table dz_c); each has its own cases after it.
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/momentum_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_momentum.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_weno_momentum.hip \
//         orthogonalsphericalshellgrids.jl_amd/csrc/tpg_weno_vi.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o momentum_argcheck
//   ./momentum_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_momentum.h"
#include "../include/tripolar_hip_weno_momentum.h"
#include "../include/tripolar_hip_weno_vi.h"

static int failures = 0;

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Args {
    const void *u, *v, *w;
    void *Gu, *Gv;
    const void* m[9];                                              // dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff, dz_f (dz_c)
    const int32_t *nfc, *ncf;
    int scheme = TPG_MOMENTUM_ENSTROPHY_CONSERVING, Nx = 48, Ny = 40, Nz = 3, Hx = 4, Hy = 4, Hz = 4, ft = TPG_F64;    // scheme: the centred call's only
};

// the three entry points behind one signature, each with the reader of its own library's last message
struct Entry {
    const char* name;
    int (*call)(const Args&);
    const char* (*last_error)(void);
};

static int centred(const Args& a)
{
    return tpg_momentum_advection_tendency(a.u, a.v, a.w, a.Gu, a.Gv, a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.m[6], a.m[7], a.m[8], a.nfc,
                                           a.ncf, 0.1, a.scheme, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static int weno(const Args& a)
{
    return tpg_weno_momentum_advection_tendency(a.u, a.v, a.w, a.Gu, a.Gv, a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.m[6], a.m[7], a.m[8], a.nfc,
                                                a.ncf, 0.1, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static int weno_vi(const Args& a)
{
    return tpg_weno_vi_momentum_advection_tendency(a.u, a.v, a.w, a.Gu, a.Gv, a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.m[6], a.m[7], a.m[8], a.nfc,
                                                   a.ncf, 0.1, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static const Entry CENTRED = { "centred", centred, tpg_momentum_last_error }, WENO = { "weno", weno, tpg_weno_momentum_last_error },
                   WENO_VI = { "weno_vi", weno_vi, tpg_weno_vi_last_error };

static void expect(const Entry& e, const Args& a, int want, const char* starts, int line)
{
    const int rc = e.call(a);
    const char* msg = e.last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d, %s: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, e.name, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(entry, args, want, starts) expect((entry), (args), (want), (starts), __LINE__)
#define EXPECT_ALL(args, want, starts) do { EXPECT(CENTRED, (args), (want), (starts)); EXPECT(WENO, (args), (want), (starts)); EXPECT(WENO_VI, (args), (want), (starts)); } while (0)

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
    // what the three calls refuse alike
    a = ok; a.ft = 7;            EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    a = ok; a.Nx = 49;           EXPECT_ALL(a, TPG_ERR_ODD_NLAMBDA, "");
    a = ok; a.v = nullptr;       EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.w = nullptr;       EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.Gv = nullptr;      EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null Gu or Gv");
    for (int q = 0; q < 9; ++q) {
        a = ok; a.m[q] = nullptr;                                   // the two older calls say dz_f, the third dz_c
        EXPECT(CENTRED, a, TPG_ERR_INVALID_ARGUMENT, "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f");
        EXPECT(WENO, a, TPG_ERR_INVALID_ARGUMENT, "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f");
        EXPECT(WENO_VI, a, TPG_ERR_INVALID_ARGUMENT, "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_c");
        a = ok; a.m[q] = at(((uintptr_t)(q + 1) << 20) + 4);
        EXPECT(CENTRED, a, TPG_ERR_INVALID_ARGUMENT, "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f pointer not aligned");
        EXPECT(WENO, a, TPG_ERR_INVALID_ARGUMENT, "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f pointer not aligned");
        EXPECT(WENO_VI, a, TPG_ERR_INVALID_ARGUMENT, "dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_c pointer not aligned");
    }
    a = ok; a.ncf = nullptr;     EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_cf is null)");
    a = ok; a.nfc = nullptr;     EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_fc is null)");
    a = ok; a.w = at(base + 2 * parent + 4);  EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "u, v or w pointer not aligned");
    a = ok; a.Gu = at(far + 2); a.ft = TPG_F32; EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "Gu or Gv pointer not aligned");
    a = ok; a.ncf = static_cast<const int32_t*>(at((21 << 20) + 2)); EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    a = ok; a.Gu = const_cast<void*>(ok.v);            EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "Gu overlaps v");
    a = ok; a.Gv = at(base + 8);                       EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps u");
    a = ok; a.Gv = at(far + parent - 8);               EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps Gu");
    a = ok; a.Gv = at(base + 2 * parent + wparent - 8); EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps w");   // the last element of w's longer parent
    a = ok; a.Gv = at(base + 2 * parent + wparent); a.Hz = 0;                 // right behind it: no overlap, the call goes on to the halo check
    EXPECT_ALL(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    Args big = ok;                                                 // refused by the plane check every entry point shares
    big.u = at(1ull << 44); big.v = at(2ull << 44); big.w = at(3ull << 44); big.Gu = at(4ull << 44); big.Gv = at(5ull << 44);
    big.nfc = big.ncf = nullptr; big.Nx = 65536; big.Ny = 32768; big.Nz = 1; big.Hz = 1; big.ft = TPG_F32;
    big.Hx = big.Hy = 1;         EXPECT(CENTRED, big, TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    big.Hx = big.Hy = 3;         EXPECT(WENO, big, TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    EXPECT(WENO_VI, big, TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    // the centred call's own: the scheme, before any pointer is looked at, and the halo of its stencil
    a = ok; a.scheme = 3;        EXPECT(CENTRED, a, TPG_ERR_UNSUPPORTED, "momentum advection scheme 3 is not built");
    a = ok; a.scheme = -1; a.u = nullptr; EXPECT(CENTRED, a, TPG_ERR_UNSUPPORTED, "momentum advection scheme -1 is not built");
    a = ok; a.Hx = 0; a.nfc = a.ncf = nullptr;
    EXPECT(CENTRED, a, TPG_ERR_UNSUPPORTED, "the rule reads u, v[i-1..i+1, j-1..j+1, k-1..k+1] and w[i-1, j], w[i, j-1]: Hx >= 1, Hy >= 1 and Hz >= 1 needed (halo (0,4,4))");
    a = ok; a.Hy = 0;            EXPECT(CENTRED, a, TPG_ERR_UNSUPPORTED, "the rule reads");
    // the WENO call's own: the halo of its stencil
    a = ok; a.Hx = 2; a.nfc = a.ncf = nullptr;
    EXPECT(WENO, a, TPG_ERR_UNSUPPORTED, "the rule reads Z[i, j-2..j+3] and Z[i-2..i+3, j], that is u, v[i-3..i+3, j-3..j+3, k-1..k+1], and w[i-1, j], w[i, j-1]: "
                                         "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,4,4))");
    a = ok; a.Hy = 2;            EXPECT(WENO, a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hx = 3; a.Hy = 3; a.Hz = 1; a.Gu = nullptr;   EXPECT(WENO, a, TPG_ERR_INVALID_ARGUMENT, "null Gu or Gv");   // the minimum halo is not refused for its halo
    // the all-upwinded call's own: the halo of its stencil
    a = ok; a.Hx = 2; a.nfc = a.ncf = nullptr;
    EXPECT(WENO_VI, a, TPG_ERR_UNSUPPORTED, "the rule reads u, v[i-3..i+3, j-3..j+3, k-3..k+3 within 0..Nz+1] and w[i-2..i+1, j], w[i, j-2..j+1]: "
                                            "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,4,4))");
    a = ok; a.Hy = 2;            EXPECT(WENO_VI, a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hx = 3; a.Hy = 3; a.Hz = 1; a.Gu = nullptr;   EXPECT(WENO_VI, a, TPG_ERR_INVALID_ARGUMENT, "null Gu or Gv");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("momentum_argcheck: every call refused in validation, as expected");
    return 0;
}
