// mixing_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_convective_adjustment_diffusivities and
// tpg_ri_based_diffusivities, for a sanitizer build of the HOST code of csrc/staged/tpg_mixing.hip (the parameter tables and their names,
// the Span records of the overlap check, the conversions to the element type) with the error channel.  The bad calls come in the order of
// the header's refusals.  Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated
// and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I orthogonalsphericalshellgrids.jl_amd/csrc -I include tools/mixing_argcheck.cpp \
//         orthogonalsphericalshellgrids.jl_amd/csrc/staged/tpg_mixing.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o mixing_argcheck
//   ./mixing_argcheck
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../orthogonalsphericalshellgrids.jl_amd/csrc/staged/tripolar_hip_mixing.h"

static int failures = 0;

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

static const unsigned long long FACES = 48ull * 40 * 7 * 8;

struct Args {
    bool ri = true;
    const void *b, *u, *v, *kprev, *nprev;
    void* out[4];                                                  // kappa_c, nu_c, kappa_u, kappa_v
    double q[6] = { 0.7, 0.5, 1.7, 0.1, 0.4, 0.6 };                // the Ri rule's; convective adjustment takes the first four
    const void* dz_f;
    const int32_t* n[3];
    double value = 0.0;
    int Nx = 48, Ny = 40, Nz = 6, Hx = 0, Hy = 0, Hz = 0, ft = TPG_F64;          // halo (0,0,0): the stencil check refuses what passes the rest
};

static Args base(bool ri)
{
    Args a;
    a.ri = ri;
    const void** in[] = { &a.b, &a.u, &a.v, &a.kprev, &a.nprev };
    for (int q = 0; q < 5; ++q) *in[q] = at((1ull << 32) + 4 * q * FACES);
    for (int q = 0; q < 4; ++q) a.out[q] = at((1ull << 36) + 4 * q * FACES);
    a.dz_f = at(5ull << 20);
    for (int q = 0; q < 3; ++q) a.n[q] = reinterpret_cast<const int32_t*>(at((6ull + q) << 20));
    return a;
}

static int call(const Args& a)
{
    if (!a.ri)
        return tpg_convective_adjustment_diffusivities(a.b, a.out[0], a.out[1], a.out[2], a.out[3], a.q[0], a.q[1], a.q[2], a.q[3], a.dz_f, a.n[0], a.n[1],
                                                       a.n[2], a.value, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
    return tpg_ri_based_diffusivities(a.b, a.u, a.v, a.kprev, a.nprev, a.out[0], a.out[1], a.out[2], a.out[3], a.q[0], a.q[1], a.q[2], a.q[3], a.q[4],
                                      a.q[5], a.dz_f, a.n[0], a.n[1], a.n[2], a.value, a.Nx, a.Ny, a.Nz, a.Hx, a.Hy, a.Hz, a.ft, nullptr);
}

static void expect(const char* what, const Args& a, int status, const char* message)
{
    const int got = call(a);
    const char* err = tpg_mixing_last_error();
    if (got != status || strncmp(err, message, strlen(message)) != 0) {
        fprintf(stderr, "%s (%s): status %d, message \"%s\" (expected %d, \"%s...\")\n", what, a.ri ? "Ri" : "convective adjustment", got, err, status, message);
        ++failures;
    }
}

int main()
{
    const int INVALID = TPG_ERR_INVALID_ARGUMENT, UNSUPPORTED = TPG_ERR_UNSUPPORTED;
    static const char* const ca_names[] = { "background_kappa", "convective_kappa", "background_nu", "convective_nu" };
    static const char* const ri_names[] = { "nu0", "kappa0", "kappa_ca", "Ri0", "Ri_delta", "Cav" };
    static const char* const out_names[] = { "kappa_c", "nu_c", "kappa_u", "kappa_v" };
    char text[160];
    for (int ri = 0; ri < 2; ++ri) {
        Args a = base(ri);
        expect("the base call", a, UNSUPPORTED, "the rule reads b, u, v and the *_prev arrays one cell west, east, south and north");
        // 1. the geometry
        a = base(ri); a.ft = 7; expect("ft", a, INVALID, "unknown element type ft=7");
        a = base(ri); a.Nx = 49; expect("odd Nx", a, TPG_ERR_ODD_NLAMBDA, "The number of cells");
        // 2. the null combinations
        a = base(ri); a.b = nullptr; expect("b", a, INVALID, "null b");
        a = base(ri); a.dz_f = nullptr; expect("dz_f", a, INVALID, "null dz_f");
        a = base(ri); for (int q = 0; q < 4; ++q) a.out[q] = nullptr;
        expect("no output", a, INVALID, "no output: kappa_c, nu_c, kappa_u and kappa_v are all null");
        // 3. the numbers, each named
        for (int q = 0; q < (ri ? 6 : 4); ++q) {
            snprintf(text, sizeof text, "%s is not finite", (ri ? ri_names : ca_names)[q]);
            a = base(ri); a.q[q] = NAN; expect("a NaN parameter", a, INVALID, text);
            a = base(ri); a.q[q] = 1e300; a.ft = TPG_F32; expect("a parameter beyond Float32", a, INVALID, text);
        }
        a = base(ri); a.value = INFINITY; expect("mask_value", a, INVALID, "mask_value is not finite");
        // 4. alignment
        a = base(ri); a.b = at((uintptr_t)a.b + 4); expect("b", a, INVALID, "b, u, v, kappa_c_prev or nu_c_prev pointer not aligned");
        a = base(ri); a.out[3] = at((uintptr_t)a.out[3] + 4); expect("kappa_v", a, INVALID, "kappa_c, nu_c, kappa_u or kappa_v pointer not aligned");
        a = base(ri); a.dz_f = at((5ull << 20) + 4); expect("dz_f", a, INVALID, "dz_f pointer not aligned to its element type");
        a = base(ri); a.n[2] = reinterpret_cast<const int32_t*>(at((8ull << 20) + 2)); expect("n_cf", a, INVALID, "count plane pointer not aligned to int32");
        // 5. the overlaps: every output against b, against the next output, against dz_f and a count plane
        for (int q = 0; q < 4; ++q) {
            snprintf(text, sizeof text, "%s overlaps b (every item reads its neighbours' cells while they write: the caller ping-pongs)", out_names[q]);
            a = base(ri); a.out[q] = at((uintptr_t)a.b + 8); expect("an output on b", a, INVALID, text);
            snprintf(text, sizeof text, "%s overlaps dz_f", out_names[q]);
            a = base(ri); a.dz_f = at((uintptr_t)a.out[q] + FACES - 8); expect("an output on dz_f", a, INVALID, text);
            snprintf(text, sizeof text, "%s overlaps n_fc", out_names[q]);
            a = base(ri); a.n[1] = reinterpret_cast<const int32_t*>(a.out[q]); expect("an output on n_fc", a, INVALID, text);
        }
        a = base(ri); a.out[2] = at((uintptr_t)a.out[1] + FACES - 8); expect("nu_c on kappa_u", a, INVALID, "nu_c overlaps kappa_u");
        // 6. the stencil, in full
        a = base(ri); a.Hy = 2; a.Hz = 3;
        expect("stencil", a, UNSUPPORTED, "the rule reads b, u, v and the *_prev arrays one cell west, east, south and north of the interior: Hx >= 1 and Hy >= 1 "
                                          "needed (halo (0,2,3))");
    }
    // the Ri call's own
    Args a = base(true); a.v = nullptr; expect("v", a, INVALID, "null u or v");
    a = base(true); a.nprev = nullptr; expect("one prev", a, INVALID, "kappa_c_prev without nu_c_prev: the time average takes both or neither");
    a = base(true); a.kprev = nullptr; expect("the other prev", a, INVALID, "nu_c_prev without kappa_c_prev: the time average takes both or neither");
    a = base(true); a.q[4] = 0.0; expect("Ri_delta", a, INVALID, "Ri_delta = 0 is not positive");
    a = base(true); a.q[5] = -1.0; expect("Cav", a, INVALID, "1 + Cav == 0: the time average divides by it");
    a = base(true); a.kprev = at((uintptr_t)a.out[0] + 16); expect("kappa_c on its prev", a, INVALID, "kappa_c overlaps kappa_c_prev");
    a = base(true); a.nprev = at((uintptr_t)a.out[3] - 16); expect("kappa_v on nu_c_prev", a, INVALID, "kappa_v overlaps nu_c_prev");
    if (failures) {
        fprintf(stderr, "mixing_argcheck: %d case(s) failed\n", failures);
        return 1;
    }
    printf("mixing_argcheck: every call refused in validation, with its status and message\n");
    return 0;
}
