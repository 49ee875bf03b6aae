// advection_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_tracer_advection_tendency, for a sanitizer build
// of the HOST code of tpg_advection.hip (the Span tables, the name formatting, the overlap arithmetic, the error channel).
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/advection_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_advection.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o advection_argcheck
//   ./advection_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_advection.h"

static int failures = 0;

static void expect(int rc, int want, const char* starts, int line)
{
    const char* msg = tpg_advection_last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(call, want, starts) expect((call), (want), (starts), __LINE__)

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

int main()
{
    const uintptr_t parent = 56ull * 48 * 11 * 8, wparent = 56ull * 48 * 12 * 8, base = 1ull << 30, far = 1ull << 40;
    void *u = at(base), *v = at(base + parent), *w = at(base + 2 * parent), *dy = at(1 << 20), *dx = at(2 << 20), *az = at(3 << 20), *dz = at(4 << 20);
    const int32_t* ncc = static_cast<const int32_t*>(at(5 << 20));
    const void* c[TPG_MAX_FIELDS + 1];
    void* G[TPG_MAX_FIELDS + 1];
    auto reset = [&] { for (int q = 0; q <= TPG_MAX_FIELDS; ++q) { c[q] = at(far + 3 * q * parent); G[q] = at(2 * far + 3 * q * parent); } };
    reset();
    auto call = [&](const void* const* c_, void* const* G_, int n, const void* u_, const void* v_, const void* w_, const void* dy_, const void* dz_,
                    const int32_t* n_, int scheme = TPG_ADVECTION_CENTERED2, int Nx = 48, int Hz = 4, int ft = TPG_F64) {
        return tpg_tracer_advection_tendency(c_, G_, n, u_, v_, w_, dy_, dx, az, dz_, n_, 0.1, scheme, Nx, 40, 3, 4, 4, Hz, ft, nullptr);
    };
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc, 0, 48, 4, 7), TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc, 0, 49), TPG_ERR_ODD_NLAMBDA, "");
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc, 3), TPG_ERR_UNSUPPORTED, "advection scheme 3 is not built");
    EXPECT(call(c, G, 0, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "no tracers (nfields = 0)");
    EXPECT(call(c, G, 17, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "17 tracers: at most TPG_MAX_FIELDS = 16");
    EXPECT(call(nullptr, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "null table");
    EXPECT(call(c, nullptr, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "null table");
    c[15] = nullptr;
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "null tracer 15");
    reset();
    G[15] = nullptr;
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "null G of tracer 15");
    reset();
    EXPECT(call(c, G, 16, u, nullptr, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    EXPECT(call(c, G, 16, u, v, w, dy, nullptr, ncc), TPG_ERR_INVALID_ARGUMENT, "null dy_fc, dx_cf, az_cc or dz_c");
    c[15] = at(far + 45 * parent + 4);                             // the last names of the tables, two digits in each
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "tracer 15: pointer not aligned");
    reset();
    G[15] = at(2 * far + 45 * parent + 2);
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc, 0, 48, 4, TPG_F32), TPG_ERR_INVALID_ARGUMENT, "G of tracer 15: pointer not aligned");
    reset();
    EXPECT(call(c, G, 16, u, v, at(base + 2 * parent + 4), dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "u, v or w pointer not aligned");
    EXPECT(call(c, G, 16, u, v, w, at((1 << 20) + 4), dz, ncc), TPG_ERR_INVALID_ARGUMENT, "dy_fc, dx_cf, az_cc or dz_c pointer not aligned");
    EXPECT(call(c, G, 16, u, v, w, dy, dz, static_cast<const int32_t*>(at((5 << 20) + 2))), TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    G[15] = const_cast<void*>(c[14]);
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps tracer 14");
    G[15] = at(2 * far + 42 * parent + parent - 8);
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps G of tracer 14");
    G[15] = at(base + 2 * parent + wparent - 8);                   // the last element of w's longer parent
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps w");
    G[15] = at(base + 2 * parent + wparent);                       // right behind it: no overlap, the call goes on to the halo check
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc, 0, 48, 0), TPG_ERR_UNSUPPORTED, "the rule reads");
    G[0] = at(base + 8);
    EXPECT(call(c, G, 16, u, v, w, dy, dz, ncc), TPG_ERR_INVALID_ARGUMENT, "G of tracer 0 overlaps u");
    reset();
    EXPECT(call(c, G, 16, u, v, w, dy, dz, nullptr, 0, 48, 0), TPG_ERR_UNSUPPORTED, "the rule reads");
    for (int q = 0; q < 16; ++q) { c[q] = at((uintptr_t)(q + 1) << 44); G[q] = at((uintptr_t)(q + 21) << 44); }
    EXPECT(tpg_tracer_advection_tendency(c, G, 16, at(41ull << 44), at(42ull << 44), at(43ull << 44), dy, dx, az, dz, nullptr, 0.0, 0, 65536, 32768, 1, 1, 1, 1,
                                         TPG_F32, nullptr), TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("advection_argcheck: every call refused in validation, as expected");
    return 0;
}
