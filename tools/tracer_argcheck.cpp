// tracer_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_tracer_advection_tendency,
// tpg_weno_tracer_advection_tendency and tpg_weno_xyz_tracer_advection_tendency, for a sanitizer build of the HOST code the three share
// (tpg_tracer_tendency.hpp: the Span tables, the name formatting, the overlap arithmetic) with the error channel.  One table of bad calls
// goes through all three entry points, in the order of the headers' refusals; each has its own cases after it.
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/tracer_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_advection.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_weno.hip \
//         orthogonalsphericalshellgrids.jl_amd/csrc/tpg_weno_xyz.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o tracer_argcheck
//   ./tracer_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_advection.h"
#include "../include/tripolar_hip_weno.h"
#include "../include/tripolar_hip_weno_xyz.h"

static int failures = 0;

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Args {
    const void* c[TPG_MAX_FIELDS + 1];
    void* G[TPG_MAX_FIELDS + 1];
    const void* const* ct;
    void* const* Gt;
    int n = 2;
    const void *u, *v, *w;
    const void* m[4];                                              // dy_fc, dx_cf, az_cc, dz_c
    const int32_t* ncc = nullptr;
    int scheme = TPG_ADVECTION_CENTERED2, Nx = 48, Ny = 40, Nz = 3, Hx = 4, Hy = 4, Hz = 4, ft = TPG_F64;    // scheme: the centred call's only
};

// the three entry points behind one signature, each with the reader of its own library's last message
struct Entry {
    const char* name;
    int (*call)(const Args&);
    const char* (*last_error)(void);
};

static int centred(const Args& a)
{
    return tpg_tracer_advection_tendency(a.ct ? a.c : nullptr, a.Gt ? a.G : nullptr, a.n, a.u, a.v, a.w, a.m[0], a.m[1], a.m[2], a.m[3], a.ncc, 0.1, a.scheme,
                                         a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static int weno(const Args& a)
{
    return tpg_weno_tracer_advection_tendency(a.ct ? a.c : nullptr, a.Gt ? a.G : nullptr, a.n, a.u, a.v, a.w, a.m[0], a.m[1], a.m[2], a.m[3], a.ncc, 0.1,
                                              a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static int weno_xyz(const Args& a)
{
    return tpg_weno_xyz_tracer_advection_tendency(a.ct ? a.c : nullptr, a.Gt ? a.G : nullptr, a.n, a.u, a.v, a.w, a.m[0], a.m[1], a.m[2], a.m[3], a.ncc,
                                                  0.1, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static const Entry CENTRED = { "centred", centred, tpg_advection_last_error }, WENO = { "weno", weno, tpg_weno_last_error },
                   WENO_XYZ = { "weno_xyz", weno_xyz, tpg_weno_xyz_last_error };

static void expect(const Entry& e, const Args& a, int want, const char* starts, const char* holds, int line)
{
    const int rc = e.call(a);
    const char* msg = e.last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0 || !std::strstr(msg, holds)) {
        std::fprintf(stderr, "line %d, %s: status %d (want %d), message \"%s\" (want \"%s...%s\")\n", line, e.name, rc, want, msg, starts, holds);
        ++failures;
    }
}
#define EXPECT(entry, args, want, starts) expect((entry), (args), (want), (starts), "", __LINE__)
#define EXPECT_HOLDS(entry, args, want, starts, holds) expect((entry), (args), (want), (starts), (holds), __LINE__)
#define EXPECT_ALL(args, want, starts) do { EXPECT(CENTRED, (args), (want), (starts)); EXPECT(WENO, (args), (want), (starts)); EXPECT(WENO_XYZ, (args), (want), (starts)); } while (0)

int main()
{
    const uintptr_t parent = 56ull * 48 * 11 * 8, wparent = 56ull * 48 * 12 * 8, base = 1ull << 30, far = 1ull << 40;
    Args ok;
    for (int q = 0; q <= TPG_MAX_FIELDS; ++q) { ok.c[q] = at(far + 3 * q * parent); ok.G[q] = at(2 * far + 3 * q * parent); }
    ok.ct = ok.c; ok.Gt = ok.G;                                    // non-null: an entry passes the tables of the copy it is given
    ok.u = at(base); ok.v = at(base + parent); ok.w = at(base + 2 * parent);
    for (int q = 0; q < 4; ++q) ok.m[q] = at((uintptr_t)(q + 1) << 20);
    Args a;
    // what the three calls refuse alike
    // 1. the geometry
    a = ok; a.ft = 7;            EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    a = ok; a.Nx = 49;           EXPECT_ALL(a, TPG_ERR_ODD_NLAMBDA, "");
    a = ok; a.Nz = 0;            EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "invalid size");
    a = ok; a.Hz = -1;           EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "invalid size");
    // 2. the number of tracers
    a = ok; a.n = 0;             EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "no tracers (nfields = 0)");
    a = ok; a.n = TPG_MAX_FIELDS + 1; EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "17 tracers: at most TPG_MAX_FIELDS = 16 in one call");
    a = ok; a.n = TPG_MAX_FIELDS; a.u = nullptr; EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");       // 16 are accepted: every Span is written
    // 3. the tables and their entries
    a = ok; a.ct = nullptr;      EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null table of tracers or of tendencies");
    a = ok; a.Gt = nullptr;      EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null table of tracers or of tendencies");
    a = ok; a.c[1] = nullptr;    EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null tracer 1");
    a = ok; a.G[0] = nullptr;    EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null G of tracer 0");
    a = ok; a.n = TPG_MAX_FIELDS; a.c[15] = nullptr; EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null tracer 15");   // the last names of the tables, two digits in each
    a = ok; a.n = TPG_MAX_FIELDS; a.G[15] = nullptr; EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null G of tracer 15");
    // 4. the velocities and the metrics
    a = ok; a.u = nullptr;       EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.v = nullptr;       EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.w = nullptr;       EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    for (int q = 0; q < 4; ++q) {
        a = ok; a.m[q] = nullptr; EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "null dy_fc, dx_cf, az_cc or dz_c");
        // 5. alignment
        a = ok; a.m[q] = at(((uintptr_t)(q + 1) << 20) + 4);
        EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "dy_fc, dx_cf, az_cc or dz_c pointer not aligned");
    }
    a = ok; a.c[1] = at(far + 3 * parent + 4);   EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "tracer 1: pointer not aligned");
    a = ok; a.G[0] = at(2 * far + 2); a.ft = TPG_F32; EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 0: pointer not aligned");
    a = ok; a.n = TPG_MAX_FIELDS; a.c[15] = at(far + 45 * parent + 4); EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "tracer 15: pointer not aligned");
    a = ok; a.n = TPG_MAX_FIELDS; a.G[15] = at(2 * far + 45 * parent + 2); a.ft = TPG_F32;
    EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 15: pointer not aligned");
    a = ok; a.w = at(base + 2 * parent + 4);     EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "u, v or w pointer not aligned");
    a = ok; a.ncc = static_cast<const int32_t*>(at((5 << 20) + 2)); EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    // 6. the overlaps
    a = ok; a.G[1] = const_cast<void*>(ok.c[0]);        EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps tracer 0");
    a = ok; a.G[0] = at(base + 8);                      EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 0 overlaps u");
    a = ok; a.G[1] = at(base + parent + 8);             EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps v");
    a = ok; a.G[1] = at(2 * far + parent - 8);          EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps G of tracer 0");
    a = ok; a.G[1] = at(base + 2 * parent + wparent - 8); EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps w");  // the last element of w's longer parent
    a = ok; a.n = TPG_MAX_FIELDS; a.G[15] = const_cast<void*>(ok.c[15]); EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps tracer 15");
    a = ok; a.n = TPG_MAX_FIELDS; a.G[15] = const_cast<void*>(ok.c[14]); EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps tracer 14");
    a = ok; a.n = TPG_MAX_FIELDS; a.G[15] = at(2 * far + 42 * parent + parent - 8);
    EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps G of tracer 14");
    a = ok; a.n = TPG_MAX_FIELDS; a.G[15] = at(base + 2 * parent + wparent - 8); a.ncc = static_cast<const int32_t*>(at(5 << 20));
    EXPECT_ALL(a, TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps w");
    a = ok; a.G[1] = at(base + 2 * parent + wparent); a.Hz = 0;               // right behind it: no overlap, the call goes on to the halo check
    EXPECT_ALL(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    // 7. the halo in z, which every stencil needs
    a = ok; a.Hz = 0;            EXPECT_ALL(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hz = 0; a.n = TPG_MAX_FIELDS; a.ncc = static_cast<const int32_t*>(at(5 << 20)); EXPECT_ALL(a, TPG_ERR_UNSUPPORTED, "the rule reads");
    // 8. more than 32 bits index: refused by the plane check every entry point shares, ahead of the work-item bounds
    Args big = ok;
    for (int q = 0; q < TPG_MAX_FIELDS; ++q) { big.c[q] = at((uintptr_t)(q + 1) << 44); big.G[q] = at((uintptr_t)(q + 21) << 44); }
    big.u = at(41ull << 44); big.v = at(42ull << 44); big.w = at(43ull << 44);
    big.Nx = 65536; big.Ny = 32768; big.Nz = 1; big.Hz = 1; big.ft = TPG_F32;
    big.n = TPG_MAX_FIELDS; big.Hx = big.Hy = 1; EXPECT(CENTRED, big, TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    big.n = 1; big.Hx = big.Hy = 3;
    EXPECT_HOLDS(WENO, big, TPG_ERR_UNSUPPORTED, "", "32-bit");
    EXPECT_HOLDS(WENO_XYZ, big, TPG_ERR_UNSUPPORTED, "", "32-bit");
    // the centred call's own: the scheme, before any pointer is looked at, and the halo of its stencil
    a = ok; a.scheme = 3; a.n = TPG_MAX_FIELDS; EXPECT(CENTRED, a, TPG_ERR_UNSUPPORTED, "advection scheme 3 is not built");
    a = ok; a.scheme = 3; a.u = nullptr;        EXPECT(CENTRED, a, TPG_ERR_UNSUPPORTED, "advection scheme 3 is not built");
    a = ok; a.Hx = 0;
    EXPECT(CENTRED, a, TPG_ERR_UNSUPPORTED, "the rule reads c[i-1..i+1, j-1..j+1, k-1..k+1], u[i+1, j] and v[i, j+1]: Hx >= 1, Hy >= 1 and Hz >= 1 needed (halo (0,4,4))");
    // the WENO calls' own: the halo of each stencil, in full
    a = ok; a.Hx = 2;
    EXPECT(WENO, a, TPG_ERR_UNSUPPORTED, "the rule reads c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-1..k+1], u[i+1, j] and v[i, j+1]: "
                                         "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,4,4))");
    EXPECT(WENO_XYZ, a, TPG_ERR_UNSUPPORTED, "the rule reads c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1], u[i+1, j] and v[i, j+1]: "
                                             "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo (2,4,4))");
    a = ok; a.Hy = 2;            EXPECT(WENO, a, TPG_ERR_UNSUPPORTED, "the rule reads"); EXPECT(WENO_XYZ, a, TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hz = 0;
    EXPECT_HOLDS(WENO, a, TPG_ERR_UNSUPPORTED, "the rule reads", "Hz >= 1 needed (halo (4,4,0))");
    EXPECT_HOLDS(WENO_XYZ, a, TPG_ERR_UNSUPPORTED, "the rule reads", "Hz >= 1 needed (halo (4,4,0))");
    a = ok; a.Hx = 3; a.Hy = 3; a.Hz = 1; a.u = nullptr;                      // the minimum halo is not refused for its halo
    EXPECT(WENO, a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w"); EXPECT(WENO_XYZ, a, TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("tracer_argcheck: every call refused in validation, as expected");
    return 0;
}
