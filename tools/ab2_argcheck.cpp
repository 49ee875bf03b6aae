// ab2_argcheck.cpp -- a stand-alone host program over the argument validation of tpg_ab2_step_velocities and tpg_ab2_step_fields, for a
// sanitizer build of the HOST code of tpg_timestep.hip (the Span tables, the name formatting, the overlap arithmetic, the error channel).
// Every call below fails in validation: none reaches a launch, no device is needed, the pointers are fabricated and never dereferenced.
// Build and run from the repository root (the sanitizers instrument the host side only; nothing of this is loaded into python or run on a GPU):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/ab2_argcheck.cpp orthogonalsphericalshellgrids.jl_amd/csrc/tpg_timestep.hip orthogonalsphericalshellgrids.jl_amd/csrc/tpg_api.hip -ldl -o ab2_argcheck
//   ./ab2_argcheck
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/tripolar_hip_timestep.h"

static int failures = 0;

static void expect(int rc, int want, const char* starts, int line)
{
    const char* msg = tpg_timestep_last_error();
    if (rc != want || std::strncmp(msg, starts, std::strlen(starts)) != 0) {
        std::fprintf(stderr, "line %d: status %d (want %d), message \"%s\" (want \"%s...\")\n", line, rc, want, msg, starts);
        ++failures;
    }
}
#define EXPECT(call, want, starts) expect((call), (want), (starts), __LINE__)

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

int main()
{
    const uintptr_t parent = 56ull * 48 * 11 * 8, base = 1ull << 30;
    void *u = at(base), *v = at(base + parent), *gun = at(base + 2 * parent), *gvn = at(base + 3 * parent), *gum = at(base + 4 * parent),
         *gvm = at(base + 5 * parent), *GU = at(base + 6 * parent), *GV = at(base + 7 * parent), *dz = at(1 << 20);
    const int32_t *nfc = static_cast<const int32_t*>(at(2 << 20)), *ncf = static_cast<const int32_t*>(at(3 << 20));
    auto vel = [&](void* u_, void* v_, void* gun_, void* gvn_, void* gum_, void* gvm_, void* GU_, void* GV_, void* dz_, const int32_t* nfc_,
                   const int32_t* ncf_, int flags, int Nx = 48, int Hy2 = 13, int ft = TPG_F64) {
        return tpg_ab2_step_velocities(u_, v_, gun_, gvn_, gum_, gvm_, GU_, GV_, dz_, nfc_, ncf_, 0.5, 0.1, flags, Nx, 40, 3, 4, 4, 4, Hy2, ft, nullptr);
    };
    const int S = TPG_AB2_STORE_PREVIOUS, E = TPG_AB2_EULER;
    EXPECT(vel(u, v, gun, gvn, gum, gvm, GU, GV, dz, nfc, ncf, S, 48, 13, 7), TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    EXPECT(vel(u, v, gun, gvn, gum, gvm, GU, GV, dz, nfc, ncf, S, 49), TPG_ERR_ODD_NLAMBDA, "");
    EXPECT(vel(u, v, gun, gvn, gum, gvm, GU, GV, dz, nfc, ncf, S, 48, -1), TPG_ERR_INVALID_ARGUMENT, "invalid north/south halo Hy2=-1");
    EXPECT(vel(u, v, gun, gvn, gum, gvm, GU, GV, dz, nfc, ncf, 12), TPG_ERR_INVALID_ARGUMENT, "unknown flag bits 0xc");
    EXPECT(vel(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dz, nullptr, nullptr, S), TPG_ERR_INVALID_ARGUMENT, "u, v, their tendencies");
    EXPECT(vel(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, GU, nullptr, dz, nullptr, nullptr, S), TPG_ERR_INVALID_ARGUMENT, "a tendency or a forcing plane");
    EXPECT(vel(u, v, nullptr, gvn, gum, gvm, GU, GV, dz, nfc, ncf, S), TPG_ERR_INVALID_ARGUMENT, "u and Gu_n must be given together");
    EXPECT(vel(u, nullptr, gun, nullptr, gum, nullptr, GU, GV, dz, nfc, ncf, S), TPG_ERR_INVALID_ARGUMENT, "Gv_m or GV given without v");
    EXPECT(vel(u, v, gun, gvn, nullptr, gvm, GU, GV, dz, nfc, ncf, S | E), TPG_ERR_INVALID_ARGUMENT, "null Gu_m");
    EXPECT(vel(u, v, gun, gvn, gum, gvm, GU, GV, nullptr, nfc, ncf, S), TPG_ERR_INVALID_ARGUMENT, "null dz_c with GU or GV given");
    EXPECT(vel(u, v, gun, gvn, gum, at(base + 5 * parent + 4), GU, GV, dz, nfc, ncf, S), TPG_ERR_INVALID_ARGUMENT, "Gv_m pointer not aligned");
    EXPECT(vel(u, v, gun, gvn, gum, gvm, GU, GV, dz, nfc, static_cast<const int32_t*>(at((3 << 20) + 2)), S), TPG_ERR_INVALID_ARGUMENT, "count plane pointer");
    EXPECT(vel(u, at(base + parent - 8), gun, gvn, gum, gvm, GU, GV, dz, nfc, ncf, S), TPG_ERR_INVALID_ARGUMENT, "u overlaps v");
    EXPECT(vel(u, v, gun, gvn, gun, gvm, GU, GV, dz, nfc, ncf, S), TPG_ERR_INVALID_ARGUMENT, "Gu_m overlaps Gu_n");
    EXPECT(vel(u, v, gun, gvn, gum, gvm, GU, at(3 << 20), dz, nfc, ncf, E), TPG_ERR_INVALID_ARGUMENT, "GV overlaps n_cf");
    EXPECT(tpg_ab2_step_velocities(at(1ull << 40), nullptr, at(1ull << 44), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.5, 0.1, E,
                                   32768, 32768, 301, 0, 0, 0, 0, TPG_F64, nullptr), TPG_ERR_UNSUPPORTED, "ab2 velocity step: too many work items");

    void* x[TPG_MAX_FIELDS + 1];
    const void* gn[TPG_MAX_FIELDS + 1];
    void* gm[TPG_MAX_FIELDS + 1];
    for (int f = 0; f <= TPG_MAX_FIELDS; ++f) { x[f] = at(base + f * parent); gn[f] = at(base + (20 + f) * parent); gm[f] = at(base + (40 + f) * parent); }
    auto fld = [&](void* const* x_, const void* const* gn_, void* const* gm_, int n, int flags, int ft = TPG_F64) {
        return tpg_ab2_step_fields(x_, gn_, gm_, n, 0.5, 0.1, flags, 48, 40, 3, 4, 4, 4, ft, nullptr);
    };
    EXPECT(fld(x, gn, gm, 16, S, 9), TPG_ERR_INVALID_ARGUMENT, "unknown element type");
    EXPECT(fld(x, gn, gm, 16, 4), TPG_ERR_INVALID_ARGUMENT, "unknown flag bits 0x4");
    EXPECT(fld(x, gn, gm, 0, S), TPG_ERR_INVALID_ARGUMENT, "no fields");
    EXPECT(fld(nullptr, gn, gm, 3, S), TPG_ERR_INVALID_ARGUMENT, "no fields");
    EXPECT(fld(x, gn, gm, 17, S), TPG_ERR_INVALID_ARGUMENT, "17 fields: at most TPG_MAX_FIELDS = 16");
    EXPECT(fld(x, gn, nullptr, 16, S), TPG_ERR_INVALID_ARGUMENT, "null Gm table");
    x[15] = nullptr;
    EXPECT(fld(x, gn, gm, 16, S), TPG_ERR_INVALID_ARGUMENT, "null field 15");
    x[15] = at(base + 15 * parent);
    gm[15] = nullptr;
    EXPECT(fld(x, gn, gm, 16, 0), TPG_ERR_INVALID_ARGUMENT, "null Gm of field 15");
    gm[15] = at(base + 55 * parent + 4);
    EXPECT(fld(x, gn, gm, 16, S), TPG_ERR_INVALID_ARGUMENT, "Gm of field 15: pointer not aligned");
    gm[15] = const_cast<void*>(gn[14]);                            // the last names of the 48-entry table, two digits in each
    EXPECT(fld(x, gn, gm, 16, S), TPG_ERR_INVALID_ARGUMENT, "Gm of field 15 overlaps Gn of field 14");
    gm[15] = at(base + 55 * parent);
    x[10] = at(base + 11 * parent - 8);
    EXPECT(fld(x, gn, gm, 16, E), TPG_ERR_INVALID_ARGUMENT, "field 10 overlaps field 11");
    x[10] = at(base + 10 * parent);
    for (int f = 0; f < 16; ++f) { x[f] = at((uintptr_t)(f + 1) << 44); gn[f] = at((uintptr_t)(f + 21) << 44); }
    EXPECT(tpg_ab2_step_fields(x, gn, nullptr, 16, 0.5, 0.1, E, 32768, 32768, 301, 0, 0, 0, TPG_F32, nullptr), TPG_ERR_UNSUPPORTED,
           "ab2 field step: too many work items");
    if (failures) { std::fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
    std::puts("ab2_argcheck: every call refused in validation, as expected");
    return 0;
}
