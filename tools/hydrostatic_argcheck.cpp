// hydrostatic_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_hydrostatic_tendencies, for a sanitizer build of
// the HOST code of libtripolar_hip_hydrostatic.so (tpg_hydrostatic.hip over tpg_operator.hpp: the Span table, the overlap arithmetic, the
// array list of chunk_plan) with the error channel, in the manner of tools/weno_vs_argcheck.cpp.  The nine refusals of the header, in its
// order.  Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never
// dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/hydrostatic_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_hydrostatic.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip \
//         -ldl -o hydrostatic_argcheck
//   ./hydrostatic_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_hydrostatic.h"

static int failures = 0;

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Args {
    const void *u, *v, *b;
    void *Gu, *Gv, *p;
    const void* m[6];                                              // f_ff, dx_fc, dy_fc, dx_cf, dy_cf, dz_f
    const int32_t *nfc, *ncf;
    int scheme = TPG_CORIOLIS_ENSTROPHY_CONSERVING, mode = TPG_TENDENCY_ADD;
    int Nx = 48, Ny = 40, Nz = 3, Hx = 4, Hy = 4, Hz = 4, ft = TPG_F64;
};

static void expect(const Args& a, int want, const char* starts, int line)
{
    const int rc = tpg_hydrostatic_tendencies(a.u, a.v, a.b, a.Gu, a.Gv, a.p, a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.nfc, a.ncf, 0.1,
                                              a.scheme, a.mode, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
    const char* msg = tpg_hydrostatic_last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(args, want, starts) expect((args), (want), (starts), __LINE__)

int main()
{
    const uintptr_t parent = 56ull * 48 * 11 * 8, base = 1ull << 30, far = 1ull << 40;
    Args ok;
    ok.u = at(base); ok.v = at(base + parent); ok.b = at(base + 2 * parent);
    ok.Gu = at(far); ok.Gv = at(far + 3 * parent); ok.p = at(far + 6 * parent);
    for (int q = 0; q < 6; ++q) ok.m[q] = at((uintptr_t)(q + 1) << 20);
    ok.nfc = static_cast<const int32_t*>(at(20 << 20));
    ok.ncf = static_cast<const int32_t*>(at(21 << 20));
    Args a;
    // 1. the geometry
    a = ok; a.ft = 7; a.scheme = 9;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    a = ok; a.Nx = 49;           EXPECT(a, TPG_ERR_ODD_NLAMBDA, "");
    a = ok; a.Nz = 0;            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "invalid size");
    // 2. the scheme, then the mode
    a = ok; a.scheme = 2; a.mode = 7; a.b = nullptr; a.m[0] = nullptr;  EXPECT(a, TPG_ERR_UNSUPPORTED, "Coriolis scheme 2 is not built");
    a = ok; a.mode = 2; a.b = nullptr; a.m[0] = nullptr;  EXPECT(a, TPG_ERR_UNSUPPORTED, "tendency mode 2 is not built");
    // 3. neither term
    a = ok; a.b = nullptr; a.m[0] = nullptr; a.Gu = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "neither f_ff nor b");
    // 4. the null combinations
    a = ok; a.Gu = nullptr; a.p = nullptr;   EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu and Gv are given together or not at all (Gu is null)");
    a = ok; a.Gv = nullptr;      EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu and Gv are given together or not at all (Gv is null)");
    a = ok; a.Gu = a.Gv = nullptr; a.p = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "without Gu and Gv the call is the pressure alone");
    a = ok; a.Gu = a.Gv = nullptr; a.b = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "without Gu and Gv the call is the pressure alone");
    a = ok; a.b = nullptr; a.m[1] = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "p_out without b");
    a = ok; a.m[1] = nullptr; a.u = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null dx_fc or dy_cf");
    a = ok; a.m[4] = nullptr;    EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null dx_fc or dy_cf");
    a = ok; a.u = nullptr; a.m[5] = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "f_ff without u, v, dx_cf or dy_fc");
    a = ok; a.v = nullptr;       EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "f_ff without u, v, dx_cf or dy_fc");
    a = ok; a.m[2] = nullptr;    EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "f_ff without u, v, dx_cf or dy_fc");
    a = ok; a.m[3] = nullptr;    EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "f_ff without u, v, dx_cf or dy_fc");
    a = ok; a.m[5] = nullptr; a.ncf = nullptr;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "b without dz_f");
    // 5. one count plane without the other
    a = ok; a.ncf = nullptr;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_cf is null)");
    a = ok; a.nfc = nullptr;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "the count planes n_fc and n_cf are given together or not at all (n_fc is null)");
    // 6. alignment
    a = ok; a.b = at(base + 2 * parent + 4);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "u, v or b pointer not aligned");
    a = ok; a.p = at(far + 6 * parent + 2); a.ft = TPG_F32;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu, Gv or p_out pointer not aligned");
    for (int q = 0; q < 6; ++q) {
        a = ok; a.m[q] = at(((uintptr_t)(q + 1) << 20) + 4);
        EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "f_ff, dx_fc, dy_fc, dx_cf, dy_cf or dz_f pointer not aligned");
    }
    a = ok; a.ncf = static_cast<const int32_t*>(at((21 << 20) + 2)); EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    // 7. the overlaps
    a = ok; a.Gu = const_cast<void*>(ok.v);            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu overlaps v");
    a = ok; a.Gv = at(base + 8);                       EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps u");
    a = ok; a.p = at(base + 3 * parent - 8);           EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "p_out overlaps b");   // the last element of b
    a = ok; a.Gv = at(far + parent - 8);               EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu overlaps Gv");
    a = ok; a.p = at(far + 4 * parent - 8);            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gv overlaps p_out");
    a = ok; a.p = at(base + 3 * parent); a.Hz = 0;     // right behind b (3 planes at Hz = 0 are shorter still): no overlap, the call goes on to the halo check
    EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    // 8. the halo
    a = ok; a.Hx = 0; a.nfc = a.ncf = nullptr;
    EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads u, v, b[i-1..i+1, j-1..j+1] and b[k..Nz+1]: Hx >= 1, Hy >= 1 and Hz >= 1 needed (halo (0,4,4))");
    a = ok; a.Hy = 0;            EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Nx = 2; a.Ny = 1; a.Nz = 1; a.Hx = a.Hy = a.Hz = 1; a.Gu = nullptr;   // the smallest shape is not refused for its geometry
    EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "Gu and Gv are given together");
    // the forms with a dropped term or without Gu, Gv pass every null check (and are refused for the halo)
    a = ok; a.Hz = 0; a.u = a.v = nullptr; a.m[0] = a.m[2] = a.m[3] = nullptr;  EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hz = 0; a.b = nullptr; a.p = nullptr; a.m[5] = nullptr;           EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hz = 0; a.Gu = a.Gv = nullptr; a.u = a.v = nullptr; for (int q = 0; q < 5; ++q) a.m[q] = nullptr;  EXPECT(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    // 9. too large for 32-bit indexing: refused by the plane check every entry point shares
    Args big = ok;
    big.u = at(1ull << 44); big.v = at(2ull << 44); big.b = at(3ull << 44); big.Gu = at(4ull << 44); big.Gv = at(5ull << 44); big.p = at(6ull << 44);
    big.nfc = big.ncf = nullptr; big.Nx = 65536; big.Ny = 32768; big.Nz = 1; big.Hx = big.Hy = big.Hz = 1; big.ft = TPG_F32;
    EXPECT(big, TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("hydrostatic_argcheck: every call refused in validation, as expected");
    return 0;
}
