// diffusion_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_diffusive_tendency, for a sanitizer build of the
// HOST code of csrc/staged/tpg_diffusion.hip (the tables of fields, tendencies and flux planes, the overlap arithmetic, the name formatting)
// with the error channel.  The bad calls come in the order of the header's refusals, with the two-digit names of a 16-field call.
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I orthogonalsphericalshellgrids.jl_amd/csrc -I include tools/diffusion_argcheck.cpp \
//         orthogonalsphericalshellgrids.jl_amd/csrc/staged/tpg_diffusion.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o diffusion_argcheck
//   ./diffusion_argcheck
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../orthogonalsphericalshellgrids.jl_amd/csrc/staged/tripolar_hip_diffusion.h"

static int failures = 0;

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Args {
    const void* c[TPG_MAX_FIELDS + 1];
    void* G[TPG_MAX_FIELDS + 1];
    const void* top[TPG_MAX_FIELDS + 1];
    const void* bottom[TPG_MAX_FIELDS + 1];
    bool ct = true, Gt = true, topt = false, bottomt = false;      // which tables are passed
    int n = 2, terms = TPG_DIFFUSION_HORIZONTAL | TPG_DIFFUSION_VERTICAL, mode = TPG_DIFFUSION_ADD, form = TPG_DIFFUSION_KAPPA_CONSTANT;
    double kh = 0.5, kz = 0.25;
    const void* kappa = nullptr;
    const void* m[7];                                              // dx_fc, dy_fc, dx_cf, dy_cf, az, dz_c, dz_f
    const int32_t* counts = nullptr;
    const void *h, *zc;
    int Nx = 48, Ny = 40, Nz = 6, Hx = 0, Hy = 0, Hz = 0, ft = TPG_F64;          // halo (0,0,0): the stencil check refuses what passes the rest
};

static const unsigned long long PARENT = 48ull * 40 * 6 * 8;

static Args base()
{
    Args a;
    for (int q = 0; q <= TPG_MAX_FIELDS; ++q) {
        a.c[q] = at((1ull << 32) + 4 * q * PARENT);
        a.G[q] = at((1ull << 36) + 4 * q * PARENT);
        a.top[q] = a.bottom[q] = nullptr;
    }
    for (int q = 0; q < 7; ++q) a.m[q] = at((7ull + q) << 20);
    a.h = at(1ull << 42);
    a.zc = at(5ull << 20);
    return a;
}

static int call(const Args& a)
{
    return tpg_diffusive_tendency(a.ct ? a.c : nullptr, a.Gt ? a.G : nullptr, a.n, a.terms, a.mode, a.kh, a.kappa, a.kz, a.form,
                                  a.topt ? a.top : nullptr, a.bottomt ? a.bottom : nullptr, a.m[0], a.m[1], a.m[2], a.m[3], a.m[4], a.m[5], a.m[6],
                                  a.counts, 0.0, a.h, a.zc, 1, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static void expect(const char* what, const Args& a, int status, const char* message)
{
    const int got = call(a);
    const char* err = tpg_diffusion_last_error();
    if (got != status || strncmp(err, message, strlen(message)) != 0) {
        fprintf(stderr, "%s: status %d, message \"%s\" (expected %d, \"%s...\")\n", what, got, err, status, message);
        ++failures;
    }
}

int main()
{
    const int INVALID = TPG_ERR_INVALID_ARGUMENT, UNSUPPORTED = TPG_ERR_UNSUPPORTED;
    Args a = base();
    expect("the base call", a, UNSUPPORTED, "the rule reads c[i-1..i+1, j, k]");
    // 1. the geometry
    a = base(); a.ft = 7; expect("ft", a, INVALID, "unknown element type ft=7");
    a = base(); a.Nx = 49; expect("odd Nx", a, TPG_ERR_ODD_NLAMBDA, "The number of cells");
    // 2. the fields
    a = base(); a.n = 0; expect("no fields", a, INVALID, "no fields (nfields = 0)");
    a = base(); a.n = TPG_MAX_FIELDS + 1; expect("too many", a, INVALID, "17 fields: at most TPG_MAX_FIELDS = 16 in one call");
    a = base(); a.ct = false; expect("null c", a, INVALID, "null table of fields or of tendencies");
    a = base(); a.Gt = false; expect("null G", a, INVALID, "null table of fields or of tendencies");
    a = base(); a.n = 16; a.c[15] = nullptr; expect("null entry", a, INVALID, "null field 15");
    a = base(); a.n = 16; a.G[12] = nullptr; expect("null G entry", a, INVALID, "null G of field 12");
    // 3. the groups
    a = base(); a.terms = 4; expect("terms", a, UNSUPPORTED, "terms 4 has bits that are not built");
    a = base(); a.terms = 0; expect("no group", a, INVALID, "no group is present");
    a = base(); a.terms = 0; a.topt = true; a.mode = 9; expect("a table is a group", a, UNSUPPORTED, "mode 9 is not built");
    // 4. the mode, then the form
    a = base(); a.mode = -1; a.form = 9; expect("mode", a, UNSUPPORTED, "mode -1 is not built (TPG_DIFFUSION_ADD = 0 and TPG_DIFFUSION_WRITE = 1 are)");
    a = base(); a.form = 3; expect("form", a, UNSUPPORTED, "kappa_z form 3 is not built");
    // 5. the null combinations
    a = base(); a.kappa = at(1ull << 43); expect("kappa with CONSTANT", a, INVALID, "kappa_z given with TPG_DIFFUSION_KAPPA_CONSTANT");
    a = base(); a.form = TPG_DIFFUSION_KAPPA_PROFILE; expect("no profile", a, INVALID, "null kappa_z with TPG_DIFFUSION_KAPPA_PROFILE");
    a = base(); a.form = TPG_DIFFUSION_KAPPA_FIELD; expect("no field", a, INVALID, "null kappa_z with TPG_DIFFUSION_KAPPA_FIELD");
    a = base(); a.m[4] = nullptr; expect("az", a, INVALID, "null dz_c or az");
    a = base(); a.m[6] = nullptr; expect("dz_f", a, INVALID, "null dz_f with TPG_DIFFUSION_VERTICAL");
    a = base(); a.m[2] = nullptr; expect("dx_cf", a, INVALID, "null dx_fc, dy_fc, dx_cf or dy_cf with TPG_DIFFUSION_HORIZONTAL");
    a = base(); a.zc = nullptr; expect("zc", a, INVALID, "bottom_height without z_centers");
    // 6. the numbers
    a = base(); a.kh = NAN; expect("kappa_h", a, INVALID, "kappa_h is not finite");
    a = base(); a.kz = INFINITY; expect("kappa_z_value", a, INVALID, "kappa_z_value is not finite");
    // 7. alignment
    a = base(); a.n = 16; a.c[11] = at((uintptr_t)a.c[11] + 4); expect("c", a, INVALID, "field 11: pointer not aligned to its element type");
    a = base(); a.n = 16; a.G[10] = at((uintptr_t)a.G[10] + 4); expect("G", a, INVALID, "G of field 10: pointer not aligned to its element type");
    a = base(); a.n = 16; a.bottomt = true; a.bottom[13] = at((1ull << 44) + 4); expect("flux", a, INVALID, "flux plane of field 13: pointer not aligned");
    a = base(); a.h = at((1ull << 42) + 4); expect("h", a, INVALID, "kappa_z, a metric plane, dz_c, dz_f, bottom_height or z_centers pointer not aligned");
    a = base(); a.counts = reinterpret_cast<const int32_t*>(at((6ull << 20) + 2)); expect("counts", a, INVALID, "count plane pointer not aligned to int32");
    // 8. the overlaps, with the names of a 16-field call
    a = base(); a.n = 16; a.G[14] = at((uintptr_t)a.c[10] + PARENT - 8);
    expect("G on c", a, INVALID, "G of field 14 overlaps field 10 (every item reads cells while its neighbours write: not an in-place call)");
    a = base(); a.n = 16; a.G[15] = at((uintptr_t)a.G[11] + 8); expect("G on G", a, INVALID, "G of field 15 overlaps G of field 11");
    a = base(); a.form = TPG_DIFFUSION_KAPPA_FIELD; a.kappa = at((uintptr_t)a.G[1] - 8); expect("G on kappa", a, INVALID, "G of field 1 overlaps kappa_z");
    a = base(); a.n = 16; a.topt = true; a.top[12] = at((uintptr_t)a.G[15] + 16); expect("G on top", a, INVALID, "G of field 15 overlaps the top flux plane of field 12");
    a = base(); a.n = 16; a.bottomt = true; a.bottom[15] = a.G[10]; expect("G on bottom", a, INVALID, "G of field 10 overlaps the bottom flux plane of field 15");
    a = base(); a.h = at((uintptr_t)a.G[1] + PARENT - 8); expect("G on h", a, INVALID, "G of field 1 overlaps bottom_height");
    // 9. the stencil, in full
    a = base(); a.Hy = 2; a.Hz = 3;
    expect("stencil", a, UNSUPPORTED, "the rule reads c[i-1..i+1, j, k], c[i, j-1..j+1, k] and the same cells of bottom_height: Hx >= 1 and Hy >= 1 needed with "
                                      "TPG_DIFFUSION_HORIZONTAL (halo (0,2,3))");
    if (failures) {
        fprintf(stderr, "diffusion_argcheck: %d case(s) failed\n", failures);
        return 1;
    }
    printf("diffusion_argcheck: every call refused in validation, with its status and message\n");
    return 0;
}
