// weno_xyz_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_weno_xyz_tracer_advection_tendency, for a sanitizer
// build of the HOST code of tpg_weno_xyz.hip (the Span tables, the overlap arithmetic, the error channel).  It drives every refusal of
// include/tripolar_hip_weno_xyz.h, in the header's order.
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/weno_xyz_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_weno_xyz.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o weno_xyz_argcheck
//   ./weno_xyz_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_weno_xyz.h"

static int failures = 0;

static void expect(int rc, int want, const char* starts, int line)
{
    const char* msg = tpg_weno_xyz_last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(call, want, starts) expect((call), (want), (starts), __LINE__)

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
    int Nx = 48, Nz = 3, Hx = 4, Hy = 4, Hz = 4, ft = TPG_F64;
};

static int call(const Args& a)
{
    return tpg_weno_xyz_tracer_advection_tendency(a.ct ? a.c : nullptr, a.Gt ? a.G : nullptr, a.n, a.u, a.v, a.w, a.m[0], a.m[1], a.m[2], a.m[3], a.ncc,
                                                  0.1, a.Nx, 40, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

int main()
{
    const uintptr_t parent = 56ull * 48 * 11 * 8, wparent = 56ull * 48 * 12 * 8, base = 1ull << 30, far = 1ull << 40;
    Args ok;
    for (int q = 0; q <= TPG_MAX_FIELDS; ++q) { ok.c[q] = at(far + 3 * q * parent); ok.G[q] = at(2 * far + 3 * q * parent); }
    ok.ct = ok.c; ok.Gt = ok.G;                                    // non-null: call() passes the tables of the copy it is given
    ok.u = at(base); ok.v = at(base + parent); ok.w = at(base + 2 * parent);
    for (int q = 0; q < 4; ++q) ok.m[q] = at((uintptr_t)(q + 1) << 20);
    Args a;
    // 1. the geometry
    a = ok; a.ft = 7;            EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    a = ok; a.Nx = 49;           EXPECT(call(a), TPG_ERR_ODD_NLAMBDA, "");
    a = ok; a.Nz = 0;            EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "invalid size");
    a = ok; a.Hz = -1;           EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "invalid size");
    // 2. the number of tracers
    a = ok; a.n = 0;             EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "no tracers (nfields = 0)");
    a = ok; a.n = TPG_MAX_FIELDS + 1; EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "17 tracers: at most TPG_MAX_FIELDS = 16 in one call");
    a = ok; a.n = TPG_MAX_FIELDS; a.u = nullptr; EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null u, v or w");          // 16 are accepted: every Span is written
    // 3. the tables and their entries
    a = ok; a.ct = nullptr;      EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null table of tracers or of tendencies");
    a = ok; a.Gt = nullptr;      EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null table of tracers or of tendencies");
    a = ok; a.c[1] = nullptr;    EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null tracer 1");
    a = ok; a.G[0] = nullptr;    EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null G of tracer 0");
    // 4. the velocities and the metrics
    a = ok; a.u = nullptr;       EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.v = nullptr;       EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    a = ok; a.w = nullptr;       EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null u, v or w");
    for (int q = 0; q < 4; ++q) {
        a = ok; a.m[q] = nullptr; EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "null dy_fc, dx_cf, az_cc or dz_c");
        // 5. alignment
        a = ok; a.m[q] = at(((uintptr_t)(q + 1) << 20) + 4);
        EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "dy_fc, dx_cf, az_cc or dz_c pointer not aligned");
    }
    a = ok; a.c[1] = at(far + 3 * parent + 4);   EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "tracer 1: pointer not aligned");
    a = ok; a.G[0] = at(2 * far + 2); a.ft = TPG_F32; EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "G of tracer 0: pointer not aligned");
    a = ok; a.w = at(base + 2 * parent + 4);     EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "u, v or w pointer not aligned");
    a = ok; a.ncc = static_cast<const int32_t*>(at((5 << 20) + 2)); EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    // 6. the overlaps
    a = ok; a.G[1] = const_cast<void*>(ok.c[0]);        EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps tracer 0");
    a = ok; a.G[0] = at(base + 8);                      EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "G of tracer 0 overlaps u");
    a = ok; a.G[1] = at(base + parent + 8);             EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps v");
    a = ok; a.G[1] = at(2 * far + parent - 8);          EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps G of tracer 0");
    a = ok; a.G[1] = at(base + 2 * parent + wparent - 8); EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "G of tracer 1 overlaps w");  // the last element of w's longer parent
    a = ok; a.n = TPG_MAX_FIELDS; a.G[15] = const_cast<void*>(ok.c[15]); EXPECT(call(a), TPG_ERR_INVALID_ARGUMENT, "G of tracer 15 overlaps tracer 15");
    a = ok; a.G[1] = at(base + 2 * parent + wparent); a.Hx = 2;               // right behind it: no overlap, the call goes on to the halo check
    EXPECT(call(a), TPG_ERR_UNSUPPORTED, "the rule reads");
    // 7. the halo, with this call's stencil text
    a = ok; a.Hx = 2;            EXPECT(call(a), TPG_ERR_UNSUPPORTED, "the rule reads c[i-3..i+3, j, k], c[i, j-3..j+3, k], c[i, j, k-3..k+3 within 0..Nz+1], u[i+1, j]");
    a = ok; a.Hy = 2;            EXPECT(call(a), TPG_ERR_UNSUPPORTED, "the rule reads");
    a = ok; a.Hz = 0;            EXPECT(call(a), TPG_ERR_UNSUPPORTED, "the rule reads");
    if (!std::strstr(tpg_weno_xyz_last_error(), "Hz >= 1 needed (halo (4,4,0))")) { std::fprintf(stderr, "halo refusal: \"%s\"\n", tpg_weno_xyz_last_error()); ++failures; }
    // 8. more work items than 32 bits index
    {
        const void* c1[1] = { at(1ull << 44) };
        void* G1[1] = { at(2ull << 44) };
        EXPECT(tpg_weno_xyz_tracer_advection_tendency(c1, G1, 1, at(3ull << 44), at(4ull << 44), at(5ull << 44), ok.m[0], ok.m[1], ok.m[2], ok.m[3], nullptr,
                                                      0.0, 65536, 32768, 1, 3, 3, 1, TPG_F32, nullptr),
               TPG_ERR_UNSUPPORTED, "");
        if (!std::strstr(tpg_weno_xyz_last_error(), "32-bit")) { std::fprintf(stderr, "32-bit refusal: \"%s\"\n", tpg_weno_xyz_last_error()); ++failures; }
    }
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("weno_xyz_argcheck: every call refused in validation, as expected");
    return 0;
}
