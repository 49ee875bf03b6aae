// tpg_value_gradient.hip -- Value / Gradient south, bottom and top halos (tpg_fill_value_gradient_halos) for gfx950.
//
// Oceananigans fills the halo of a Value- or Gradient-class condition by extrapolating linearly from the adjacent interior cell through
// the boundary face, and writes ONLY the first halo point of the side (fill_halo_regions_value_gradient.jl [recalled], parity unpinned).
// 1-based, every operation in the field's type T, in exactly this order (-ffp-contract=off: no contraction, no fma):
//     south   c[i, 0, k]    = c[i, 1, k]  + D * (-d)   d = dy_cf[i, 1]    every i of the padded row, k = 1..Nz
//     bottom  c[i, j, 0]    = c[i, j, 1]  + D * (-d)   d = dz_bottom      every (i, j) of the padded plane
//     top     c[i, j, Nz+1] = c[i, j, Nz] + D * d      d = dz_top         every (i, j) of the padded plane
// with D = (c[1] - v) / (d / 2) (top: (v - c[Nz]) / (d / 2)) for Value and D = g for Gradient.  The south pass runs before the no-flux
// mirror (tpg_fill_bounded_halos), the bottom / top pass after it: two launches, since the mirror sits between them.  No cell that a
// launch reads (plane 1 / Nz, row 1, the condition and metric rows) is one it writes, so each launch is race-free.
//
// HBM-bound and elementwise.  A work item is one 16-B chunk of one destination row; grid.y = field (wave-uniform table reads).  A field's
// rows are, in the south pass, its Nz row-0 rows (one per interior level) and, in the z pass, the sy rows of its bottom halo plane followed
// by the sy rows of its top halo plane.  Source, destination, condition and dy_cf rows of a chunk share their column offset, so the
// plain form (every row on the 16-B grid) moves aligned 16-B vectors and the GEN form (element-aligned 16-B chunks, the last chunk of a
// row moved back to end at the row's end: Float32 rows of 3610 at halo 5, offset pointers, rows shorter than a chunk) serves the rest; an
// overlapping chunk computes the same values from the same sources.
#include "tpg_launch.hpp"

namespace {

struct VGTable {
    void* ptr[TPG_MAX_FIELDS];
    const void* cond[TPG_MAX_FIELDS][2];   // slot 0: south (south pass) or bottom (z pass), slot 1: top; nullptr: the scalar value
    double value[TPG_MAX_FIELDS][2];       // scalar conditions (T values held in a double)
    int kind[TPG_MAX_FIELDS][2];           // 0, TPG_BC_VALUE or TPG_BC_GRADIENT; 0 where the pass or the geometry excludes the side
};

struct VGArgs {
    int sx, sy, Nz, Hy, Hz;
    int cpr;                               // chunks per row
    long long plane;                       // sx * sy
    int south;                             // 1: south pass, 0: bottom / top pass
    const void* dy;                        // south pass: row j = 1 of dy_cf
    double dz[2];                          // z pass: dz_bottom, dz_top (T values)
};

template <typename T, int W, bool GEN>
__global__ __launch_bounds__(256) void k_value_gradient(VGTable t, VGArgs a)
{
    typedef typename Vec<T, W>::aligned_t vec_t;
    typedef typename Vec<T, W>::loose_t lvec_t;
    typedef typename std::conditional<GEN, lvec_t, vec_t>::type cvec_t;
    const int f = blockIdx.y;
    const int k0 = t.kind[f][0], k1 = t.kind[f][1];
    const int n0 = k0 ? (a.south ? a.Nz : a.sy) : 0;
    const int rows = n0 + (k1 ? a.sy : 0);                         // the south pass has no slot 1
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= rows * a.cpr) return;
    const int r = item / a.cpr;
    const int ch = item - r * a.cpr;
    const bool top = r >= n0;
    int pd, ps, jd, js, jc;                                        // destination / source plane and row, condition row (0-based)
    if (a.south)   { pd = ps = a.Hz + r; jd = a.Hy - 1; js = a.Hy; jc = r; }
    else if (!top) { pd = a.Hz - 1; ps = a.Hz; jd = js = jc = r; }
    else           { pd = a.Hz + a.Nz; ps = a.Hz + a.Nz - 1; jd = js = jc = r - n0; }
    const int e0 = GEN ? min(ch * W, a.sx - W) : ch * W;
    const int kind = top ? k1 : k0;
    const T* cp = static_cast<const T*>(top ? t.cond[f][1] : t.cond[f][0]);
    T* c = static_cast<T*>(t.ptr[f]);
    const cvec_t s = *reinterpret_cast<const cvec_t*>(c + a.plane * ps + (long long)a.sx * js + e0);
    const cvec_t v = cp ? *reinterpret_cast<const cvec_t*>(cp + (long long)a.sx * jc + e0)
                        : (cvec_t)((T)(top ? t.value[f][1] : t.value[f][0]));
    const cvec_t d = a.south ? *reinterpret_cast<const cvec_t*>(static_cast<const T*>(a.dy) + e0)
                             : (cvec_t)((T)(top ? a.dz[1] : a.dz[0]));
    cvec_t out;
    if (kind == TPG_BC_VALUE) {
        const cvec_t half = d / (T)2;
        out = top ? s + ((v - s) / half) * d : s + ((s - v) / half) * (-d);
    } else {
        out = top ? s + v * d : s + v * (-d);
    }
    *reinterpret_cast<cvec_t*>(c + a.plane * pd + (long long)a.sx * jd + e0) = out;
}

}  // namespace

extern "C" {

int tpg_fill_value_gradient_halos(void* const fields[], int nfields, int pass, const uint8_t kinds[], const double values[],
                                  const void* const conditions[], const void* dy_cf, double dz_bottom, double dz_top,
                                  int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc) return rc;
    if (!kinds || !values || !conditions) { tpg::set_error("null kinds, values or conditions table"); return TPG_ERR_INVALID_ARGUMENT; }
    const int zbits = TPG_SIDE_BOTTOM | TPG_SIDE_TOP;
    if (pass != TPG_SIDE_SOUTH && ((pass & ~zbits) || !(pass & zbits))) {
        // south and bottom / top sit on either side of the no-flux mirror: never one call
        tpg::set_error("pass = %d: TPG_SIDE_SOUTH alone, or TPG_SIDE_BOTTOM and / or TPG_SIDE_TOP", pass);
        return TPG_ERR_INVALID_ARGUMENT;
    }
    const bool south = pass == TPG_SIDE_SOUTH;
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    // the table slots this pass uses (side 0 south, 1 bottom, 2 top), none where the axis has no halo
    int side[2] = { -1, -1 };
    if (south) { if (Hy > 0) side[0] = 0; }
    else if (Hz > 0) { if (pass & TPG_SIDE_BOTTOM) side[0] = 1; if (pass & TPG_SIDE_TOP) side[1] = 2; }
    bool any_south = false;
    for (int f = 0; f < nfields; ++f) {
        if ((uintptr_t)fields[f] % esz) { tpg::set_error("field %d: pointer not aligned to its element type", f); return TPG_ERR_INVALID_ARGUMENT; }
        for (int s = 0; s < 3; ++s) {
            const int k = kinds[3 * f + s];
            if (k != 0 && k != TPG_BC_VALUE && k != TPG_BC_GRADIENT) {
                tpg::set_error("field %d side %d: unknown kind %d (0, TPG_BC_VALUE or TPG_BC_GRADIENT)", f, s, k);
                return TPG_ERR_INVALID_ARGUMENT;
            }
            if (k && (uintptr_t)conditions[3 * f + s] % esz) {
                tpg::set_error("field %d side %d: condition pointer not aligned to its element type", f, s);
                return TPG_ERR_INVALID_ARGUMENT;
            }
        }
        any_south |= kinds[3 * f] != 0;
    }
    if (south && any_south) {
        if (!dy_cf || (uintptr_t)dy_cf % esz) { tpg::set_error("south Value / Gradient pass needs an element-aligned dy_cf"); return TPG_ERR_INVALID_ARGUMENT; }
        // row 1 must be an interior row that the horizontal fill does not write (the zipper writes row Ny)
        if (Ny < 2) { tpg::set_error("south Value / Gradient pass needs Ny >= 2 (Ny = %d)", Ny); return TPG_ERR_UNSUPPORTED; }
    }
    // the fields with a side in this pass, in order
    int active = 0;
    for (int f = 0; f < nfields; ++f)
        for (int q = 0; q < 2; ++q)
            if (side[q] >= 0 && kinds[3 * f + side[q]]) { ++active; break; }
    if (!active) return TPG_OK;
    Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    // plain 16-B chunks where every row starts on the 16-B grid, element-aligned 16-B (or, for rows shorter than 16 B, 8-B) chunks otherwise
    const int WMAX = (int)(16 / esz);
    bool plain = rows_on_16B_grid((size_t)g.sx * esz, nullptr, 0, south ? dy_cf : nullptr);
    for (int f = 0; f < nfields && plain; ++f)
        for (int q = 0; q < 2; ++q)
            if (side[q] >= 0 && kinds[3 * f + side[q]])
                plain = plain && rows_on_16B_grid(0, nullptr, 0, fields[f], conditions[3 * f + side[q]]);
    const int W = plain || g.sx >= WMAX ? WMAX : 2;
    const int cpr = plain ? g.sx / W : (g.sx + W - 1) / W;
    const long long max_rows = south ? (long long)Nz : 2ll * g.sy;
    if (max_rows * cpr >= (1ll << 31) - 256) {
        tpg::set_error("Value / Gradient halos too large for 32-bit work-item indexing");
        return TPG_ERR_UNSUPPORTED;
    }
    VGArgs a{ g.sx, g.sy, Nz, Hy, Hz, cpr, g.plane, south ? 1 : 0,
              south ? static_cast<const void*>(static_cast<const char*>(dy_cf) + (size_t)Hy * g.sx * esz) : nullptr, { dz_bottom, dz_top } };
    hipStream_t s = tpg::as_stream(stream);
    int f = 0;
    while (f < nfields) {
        VGTable t;
        int n = 0;
        long long rows = 0;
        for (; f < nfields && n < TPG_MAX_FIELDS; ++f) {
            int k[2] = { 0, 0 };
            for (int q = 0; q < 2; ++q)
                if (side[q] >= 0) k[q] = kinds[3 * f + side[q]];
            if (!k[0] && !k[1]) continue;
            t.ptr[n] = fields[f];
            for (int q = 0; q < 2; ++q) {
                t.kind[n][q] = k[q];
                t.cond[n][q] = k[q] ? conditions[3 * f + side[q]] : nullptr;
                t.value[n][q] = k[q] ? values[3 * f + side[q]] : 0.0;
            }
            const long long rf = south ? Nz : (k[0] ? (long long)g.sy : 0) + (k[1] ? (long long)g.sy : 0);
            rows = rf > rows ? rf : rows;
            ++n;
        }
        if (n == 0) break;
        dim3 grid((unsigned)((rows * cpr + 255) / 256), (unsigned)n);
        dispatch_ft(ft, [&](auto ty) {
            dispatch_chunk<decltype(ty)>(W, !plain, [&](auto w, auto gen) {
                hipLaunchKernelGGL((k_value_gradient<decltype(ty), decltype(w)::value, decltype(gen)::value>), grid, dim3(256), 0, s, t, a);
            });
        });
        if ((rc = tpg::launch_status("k_value_gradient"))) return rc;
    }
    return TPG_OK;
}

}  // extern "C"
