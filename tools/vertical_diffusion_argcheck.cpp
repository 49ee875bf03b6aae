// vertical_diffusion_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_vertical_implicit_diffusion, for a
// sanitizer build of the HOST code of libtripolar_hip_vertical_diffusion.so (tpg_vertical_diffusion.hip over tpg_operator.hpp: the Span table
// of up to eighteen arrays, the overlap arithmetic, the array list of chunk_plan) with the error channel, in the manner of
// tools/hydrostatic_argcheck.cpp.  The nine refusals of the header, in its order.  Every call below fails in validation: none reaches a
// launch, no device is needed, the pointers are fabricated and never dereferenced.  A call that passes a check is one of 200 levels on the
// on-chip path: it is refused for the on-chip bound, the eighth check.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/vertical_diffusion_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_vertical_diffusion.hip \
//         orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o vertical_diffusion_argcheck
//   ./vertical_diffusion_argcheck
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_vertical_diffusion.h"

static int failures = 0;

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Args {
    void* fields[TPG_MAX_FIELDS + 1];
    void* const* table = fields;
    int n = 3;
    const void* kappa = nullptr;
    double kappa_value = 0.5, dt = 0.7;
    int form = TPG_KAPPA_CONSTANT, path = TPG_VDIFF_ON_CHIP;
    const void *dzc, *dzf;
    const int32_t* counts;
    void* scratch = nullptr;
    int Nx = 48, Ny = 40, Nz = 200, Hx = 4, Hy = 4, Hz = 4, ft = TPG_F64;
};

static void expect(const Args& a, int want, const char* starts, int line)
{
    const int rc = tpg_vertical_implicit_diffusion(a.table == nullptr ? nullptr : a.fields, a.n, a.kappa, a.kappa_value, a.form, a.dzc, a.dzf, a.counts,
                                                   0.0, a.dt, a.scratch, a.path, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
    const char* msg = tpg_vertical_diffusion_last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(args, want, starts) expect((args), (want), (starts), __LINE__)

int main()
{
    const uintptr_t parent = 56ull * 48 * 208 * 8, base = 1ull << 32, far = 1ull << 42;
    const char* bound = "Nz = 200 is beyond the on-chip path's 160 levels";
    Args ok;
    for (int f = 0; f <= TPG_MAX_FIELDS; ++f) ok.fields[f] = at(base + f * parent);
    ok.dzc = at(1 << 20); ok.dzf = at(2 << 20);
    ok.counts = static_cast<const int32_t*>(at(3 << 20));
    void* const kappa = at(far);
    void* const scratch = at(far + 4 * parent);
    Args a;
    EXPECT(ok, TPG_ERR_UNSUPPORTED, bound);                        // the base call passes the first seven checks
    // 1. the geometry
    a = ok; a.ft = 7; a.n = 0;   EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    a = ok; a.Nx = 49;           EXPECT(a, TPG_ERR_ODD_NLAMBDA, "");
    a = ok; a.Nz = 0;            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "invalid size");
    // 2. the fields
    a = ok; a.n = 0; a.form = 9; EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "no fields");
    a = ok; a.table = nullptr;   EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "no fields");
    a = ok; a.n = TPG_MAX_FIELDS + 1;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "17 fields: at most TPG_MAX_FIELDS = 16");
    a = ok; a.fields[2] = nullptr;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null field 2");
    a = ok; a.n = TPG_MAX_FIELDS;      EXPECT(a, TPG_ERR_UNSUPPORTED, bound);     // sixteen fields fill the Span table
    // 3. the form, then the path
    a = ok; a.form = 3; a.path = 7;    EXPECT(a, TPG_ERR_UNSUPPORTED, "kappa form 3 is not built");
    a = ok; a.path = 3; a.dzc = nullptr;  EXPECT(a, TPG_ERR_UNSUPPORTED, "path 3 is not built");
    // 4. the null combinations
    a = ok; a.kappa = kappa;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "kappa given with TPG_KAPPA_CONSTANT");
    a = ok; a.form = TPG_KAPPA_PROFILE;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null kappa with TPG_KAPPA_PROFILE");
    a = ok; a.form = TPG_KAPPA_FIELD;    EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null kappa with TPG_KAPPA_FIELD");
    a = ok; a.dzc = nullptr;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null dz_c or dz_f");
    a = ok; a.dzf = nullptr;     EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "null dz_c or dz_f");
    a = ok; a.path = TPG_VDIFF_STREAMED; a.dt = NAN;  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "TPG_VDIFF_STREAMED without scratch");
    // 5. the step and the constant
    a = ok; a.dt = INFINITY; a.fields[0] = at(base + 4);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "dt is not finite");
    a = ok; a.kappa_value = NAN; EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "kappa_value is not finite");
    a = ok; a.kappa_value = NAN; a.form = TPG_KAPPA_PROFILE; a.kappa = kappa;  EXPECT(a, TPG_ERR_UNSUPPORTED, bound);    // not read in the other forms
    // 6. alignment
    a = ok; a.fields[1] = at(base + parent + 4);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "field 1: pointer not aligned");
    a = ok; a.ft = TPG_F32; a.fields[2] = at(base + 2 * parent + 2);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "field 2: pointer not aligned");
    a = ok; a.dzf = at((2 << 20) + 4);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "kappa, dz_c, dz_f or scratch pointer not aligned");
    a = ok; a.scratch = at(far + 4 * parent + 4);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "kappa, dz_c, dz_f or scratch pointer not aligned");
    a = ok; a.counts = static_cast<const int32_t*>(at((3 << 20) + 2));  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    // 7. the overlaps
    a = ok; a.fields[2] = at(base + 8);            EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "field 0 overlaps field 2");
    a = ok; a.scratch = at(base + 3 * parent - 8); EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "field 2 overlaps scratch");     // the last element of field 2
    a = ok; a.form = TPG_KAPPA_FIELD; a.kappa = at(base + parent);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "field 1 overlaps kappa");
    a = ok; a.form = TPG_KAPPA_FIELD; a.kappa = kappa; a.scratch = at(far + parent - 8);  EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "scratch overlaps kappa");
    a = ok; a.form = TPG_KAPPA_PROFILE; a.kappa = kappa; a.scratch = at(far - 8);         EXPECT(a, TPG_ERR_INVALID_ARGUMENT, "scratch overlaps kappa");
    a = ok; a.form = TPG_KAPPA_PROFILE; a.kappa = at(base + 16);  EXPECT(a, TPG_ERR_UNSUPPORTED, bound);    // a profile is only read: not checked against the fields
    a = ok; a.scratch = at(base + 3 * parent);     EXPECT(a, TPG_ERR_UNSUPPORTED, bound);                   // right behind field 2: no overlap
    // 8. the on-chip bound: on the on-chip path, and on AUTO without scratch
    a = ok; a.path = TPG_VDIFF_AUTO;  EXPECT(a, TPG_ERR_UNSUPPORTED, bound);
    a = ok; a.Nz = 161;               EXPECT(a, TPG_ERR_UNSUPPORTED, "Nz = 161 is beyond the on-chip path's 160 levels");
    if (tpg_vertical_diffusion_on_chip_levels(1, TPG_F64) != 160 || tpg_vertical_diffusion_on_chip_levels(16, TPG_F32) != 160 ||
        tpg_vertical_diffusion_on_chip_levels(0, TPG_F64) != TPG_ERR_INVALID_ARGUMENT || tpg_vertical_diffusion_on_chip_levels(1, 5) != TPG_ERR_INVALID_ARGUMENT) {
        std::fprintf(stderr, "tpg_vertical_diffusion_on_chip_levels\n");
        ++failures;
    }
    // 9. too large for 32-bit indexing: refused by the plane check every entry point shares
    Args big = ok;
    for (int f = 0; f < 3; ++f) big.fields[f] = at((uintptr_t)(f + 1) << 44);
    big.counts = nullptr; big.Nx = 65536; big.Ny = 32768; big.Nz = 1; big.Hx = big.Hy = big.Hz = 1; big.ft = TPG_F32;
    EXPECT(big, TPG_ERR_UNSUPPORTED, "horizontal plane too large");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("vertical_diffusion_argcheck: every call refused in validation, as expected");
    return 0;
}
