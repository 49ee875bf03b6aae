// tpg_open.hip -- Open (impenetrable) south, bottom and top faces of wall-normal velocities (tpg_fill_open_faces) for gfx950.
//
// Oceananigans writes the boundary-normal velocity of an Open-class condition (OpenBoundaryCondition(v); ImpenetrableBoundaryCondition()
// = BoundaryCondition(Open(), nothing)) ON THE BOUNDARY FACE ITSELF, which for a Face-located field is an interior cell, and touches no
// halo cell for that side; it does so before every other pass of fill_halo_regions! (fill_open_boundary_regions! [recalled], parity
// unpinned).  1-based, Nz the field's own level count (grid Nz + 1 for a ZFaceField):
//     south   c[i, 1, k]  = v     k = 1..Nz      a field at (Center, Face, Center)
//     bottom  c[i, j, 1]  = v     j = 1..Ny      a field at (Center, Center, Face)
//     top     c[i, j, Nz] = v     j = 1..Ny      a field at (Center, Center, Face)
// v = 0 for an impenetrable side, otherwise the prescribed normal velocity in the field's type.  A PRE-PASS: it runs before the horizontal
// fill of the same fields, which folds the written rows into the north halo and carries them into the x halos; periodic x always follows,
// so this pass writes all Nx + 2 Hx columns of each row it owns (rows 1..Ny of a face plane are one contiguous block) and the x-halo part is
// overwritten before anyone reads it.  Rows j <= 0 and j > Ny of the face planes, planes k <= 0 and k >= Nz + 1 are not written.
// Unpinned: a second reading of Oceananigans puts the face write inside the regular south / bottom-top kernels.  Both write the face cell
// only and agree on the final parent for a scalar v whenever the field's other sides are a model's defaults; they can differ only (a) in
// rows j <= 0 of the two face planes of a w field whose south side has no condition and (b) in what the halo entries of an array-valued
// condition mean.  This file implements the first reading.  Where one field carries south AND bottom / top (no Oceananigans location
// does), the cells both own, c[i, 1, 1] and c[i, 1, Nz], take the z side's value: the south rows of such a field skip those levels.
//
// HBM-bound stores (plus one load per cell of an array condition), no arithmetic.  A work item is one 16-B chunk of one destination row;
// grid.y = field (wave-uniform table reads); a field's rows are its south rows (one per level), then rows 1..Ny of its bottom face plane,
// then rows 1..Ny of its top face plane.  Condition and destination rows of a chunk share their column offset, so the plain form (field
// AND condition rows on the 16-B grid) moves aligned 16-B vectors and the GEN form (element-aligned 16-B chunks, the last chunk of a row
// moved back to end at the row's end: Float32 rows of 3610 at halo 5, offset pointers, rows shorter than a chunk) serves the rest; an
// overlapping chunk writes the same values.  Every lane of a wave runs the same instructions: the side of a row only selects addresses.
//
// The stores are ordinary (no non-temporal hint).  The horizontal fill reads part of what this pass writes right behind it, so the hint was
// measured, not guessed: -DTPG_OPEN_NT=1 compiles the hinted form; over the whole (u, v, w, T, S) fill at 3600 x 1800 x 75 the two forms are
// equal within the run-to-run spread, and the pass alone is faster with ordinary stores at Float64 (22.8 against 28.3 us at halo 5) and within
// 1 us either way at Float32 (profiles/open/nt_ab.json).
#include "tpg_launch.hpp"

#ifndef TPG_OPEN_NT
#define TPG_OPEN_NT 0
#endif

namespace {

struct OpenTable {
    void* ptr[TPG_MAX_FIELDS];
    const void* cond[TPG_MAX_FIELDS][3];   // south, bottom, top; nullptr: the scalar value
    double value[TPG_MAX_FIELDS][3];       // scalar conditions (T values held in a double)
    int sides[TPG_MAX_FIELDS];             // TPG_SIDE_* bits
};

struct OpenArgs {
    int sx, Ny, Nz, Hy, Hz;
    int cpr;                               // chunks per row
    long long plane;                       // sx * sy
};

template <typename T, int W, bool GEN>
__global__ __launch_bounds__(256) void k_open_faces(OpenTable t, OpenArgs a)
{
    typedef typename Vec<T, W>::aligned_t vec_t;
    typedef typename Vec<T, W>::loose_t lvec_t;
    typedef typename std::conditional<GEN, lvec_t, vec_t>::type cvec_t;
    const int f = blockIdx.y;
    const int sides = t.sides[f];
    const int kb = (sides & TPG_SIDE_BOTTOM) ? 1 : 0, kt = (sides & TPG_SIDE_TOP) ? 1 : 0;
    const int ns = (sides & TPG_SIDE_SOUTH) ? a.Nz - kb - kt : 0;  // levels 1 / Nz of a field with a z side are that side's
    const int nb = kb ? a.Ny : 0;
    const int rows = ns + nb + (kt ? a.Ny : 0);
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= rows * a.cpr) return;
    const int r = item / a.cpr;
    const int ch = item - r * a.cpr;
    // the three table entries of the field are wave-uniform (scalar) reads; the row's side only selects among them
    const void *c0 = t.cond[f][0], *c1 = t.cond[f][1], *c2 = t.cond[f][2];
    const double v0 = t.value[f][0], v1 = t.value[f][1], v2 = t.value[f][2];
    int pd, jd, jc;                                                // destination plane and row, condition row (0-based)
    const T* cp;
    T sv;
    if (r < ns)           { cp = static_cast<const T*>(c0); sv = (T)v0; pd = a.Hz + kb + r; jd = a.Hy; jc = kb + r; }
    else if (r < ns + nb) { cp = static_cast<const T*>(c1); sv = (T)v1; pd = a.Hz; jd = jc = a.Hy + r - ns; }
    else                  { cp = static_cast<const T*>(c2); sv = (T)v2; pd = a.Hz + a.Nz - 1; jd = jc = a.Hy + r - ns - nb; }
    const int e0 = GEN ? min(ch * W, a.sx - W) : ch * W;
    const cvec_t v = cp ? *reinterpret_cast<const cvec_t*>(cp + (long long)a.sx * jc + e0) : (cvec_t)(sv);
    cvec_t* dst = reinterpret_cast<cvec_t*>(static_cast<T*>(t.ptr[f]) + a.plane * pd + (long long)a.sx * jd + e0);
#if TPG_OPEN_NT
    __builtin_nontemporal_store(v, dst);
#else
    *dst = v;
#endif
}

}  // namespace

extern "C" {

int tpg_fill_open_faces(void* const fields[], int nfields, const uint8_t sides[], const double values[], const void* const conditions[],
                        int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc) return rc;
    if (!sides || !values || !conditions) { tpg::set_error("null sides, values or conditions table"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    const int bit[3] = { TPG_SIDE_SOUTH, TPG_SIDE_BOTTOM, TPG_SIDE_TOP };
    const int all = TPG_SIDE_SOUTH | TPG_SIDE_BOTTOM | TPG_SIDE_TOP;
    int active = 0;
    bool both_z = false;
    int any = 0;
    for (int f = 0; f < nfields; ++f) {
        if (sides[f] & ~all) { tpg::set_error("field %d: sides = %d has bits other than TPG_SIDE_SOUTH | TPG_SIDE_BOTTOM | TPG_SIDE_TOP", f, (int)sides[f]); return TPG_ERR_INVALID_ARGUMENT; }
        if ((uintptr_t)fields[f] % esz) { tpg::set_error("field %d: pointer not aligned to its element type", f); return TPG_ERR_INVALID_ARGUMENT; }
        for (int s = 0; s < 3; ++s)
            if ((sides[f] & bit[s]) && (uintptr_t)conditions[3 * f + s] % esz) {
                tpg::set_error("field %d side %d: condition pointer not aligned to its element type", f, s);
                return TPG_ERR_INVALID_ARGUMENT;
            }
        any |= sides[f];
        active += sides[f] != 0;
        both_z |= (sides[f] & TPG_SIDE_BOTTOM) && (sides[f] & TPG_SIDE_TOP);
    }
    // row 1 must be an interior row that the horizontal fill does not write (the zipper writes row Ny)
    if ((any & TPG_SIDE_SOUTH) && Ny < 2) { tpg::set_error("south Open face needs Ny >= 2 (Ny = %d)", Ny); return TPG_ERR_UNSUPPORTED; }
    if (both_z && Nz < 2) { tpg::set_error("bottom and top Open faces of one field need Nz >= 2 (Nz = %d): they are one plane", Nz); return TPG_ERR_UNSUPPORTED; }
    Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    // plain 16-B chunks where every field and condition row starts on the 16-B grid, element-aligned 16-B (or, for rows shorter than 16 B,
    // 8-B) chunks otherwise
    const int WMAX = (int)(16 / esz);
    bool plain = rows_on_16B_grid((size_t)g.sx * esz, nullptr, 0);
    for (int f = 0; f < nfields && plain; ++f) {
        if (!sides[f]) continue;
        plain = rows_on_16B_grid(0, nullptr, 0, fields[f]);
        for (int s = 0; s < 3 && plain; ++s)
            if (sides[f] & bit[s]) plain = rows_on_16B_grid(0, nullptr, 0, conditions[3 * f + s]);
    }
    const int W = plain || g.sx >= WMAX ? WMAX : 2;
    const int cpr = plain ? g.sx / W : (g.sx + W - 1) / W;
    if (((long long)Nz + 2ll * Ny) * cpr >= (1ll << 31) - 256) {
        tpg::set_error("Open faces too large for 32-bit work-item indexing");
        return TPG_ERR_UNSUPPORTED;
    }
    if (!active) return TPG_OK;
    OpenArgs a{ g.sx, Ny, Nz, Hy, Hz, cpr, g.plane };
    hipStream_t st = tpg::as_stream(stream);
    int f = 0;
    while (f < nfields) {
        OpenTable t;
        int n = 0;
        long long rows = 0;
        for (; f < nfields && n < TPG_MAX_FIELDS; ++f) {
            if (!sides[f]) continue;
            t.ptr[n] = fields[f];
            t.sides[n] = sides[f];
            for (int s = 0; s < 3; ++s) {
                const bool on = (sides[f] & bit[s]) != 0;
                t.cond[n][s] = on ? conditions[3 * f + s] : nullptr;
                t.value[n][s] = on ? values[3 * f + s] : 0.0;
            }
            const int kz = ((sides[f] & TPG_SIDE_BOTTOM) ? 1 : 0) + ((sides[f] & TPG_SIDE_TOP) ? 1 : 0);
            const long long rf = ((sides[f] & TPG_SIDE_SOUTH) ? (long long)Nz - kz : 0) + (long long)kz * Ny;
            rows = rf > rows ? rf : rows;
            ++n;
        }
        if (n == 0) break;                                           // a field with a side has at least one row: rows >= 1 here
        dim3 grid((unsigned)((rows * cpr + 255) / 256), (unsigned)n);
        dispatch_ft(ft, [&](auto ty) {
            dispatch_chunk<decltype(ty)>(W, !plain, [&](auto w, auto gen) {
                hipLaunchKernelGGL((k_open_faces<decltype(ty), decltype(w)::value, decltype(gen)::value>), grid, dim3(256), 0, st, t, a);
            });
        });
        if ((rc = tpg::launch_status("k_open_faces"))) return rc;
    }
    return TPG_OK;
}

}  // extern "C"
