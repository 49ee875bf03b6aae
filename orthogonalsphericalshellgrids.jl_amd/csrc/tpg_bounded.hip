// tpg_bounded.hip -- no-flux mirror of the south, bottom and top halos (tpg_fill_bounded_halos) for gfx950.
//
// Oceananigans fills the halo of every Flux-class boundary condition as a no-flux mirror, whatever the flux value
// (fill_halo_regions_flux.jl [recalled]; the flux itself enters the tendency).  The reference keeps those conditions on the south,
// bottom and top sides of its fields and replaces only the north side (src/tripolar_grid_extensions.jl:25-44, 57-80).  1-based:
//     south   c[i, 1-j, k]  = c[i, j, k]        j = 1..Hy, every i of the padded row, k = 1..Nz
//     bottom  c[i, j, 1-k]  = c[i, j, k]        k = 1..Hz, every (i, j) of the padded plane
//     top     c[i, j, Nz+k] = c[i, j, Nz+1-k]   k = 1..Hz, every (i, j) of the padded plane
// applied after the horizontal fill, south first.  Every written cell is read from a cell that this launch does not write: the
// south-and-bottom (top) corner c[i, 1-j, 1-k] takes c[i, j, k] directly (the composed map), so the one launch is race-free.
//
// HBM-bound row copies, no arithmetic.  A work item is one 16-B chunk of one destination row; the rows of a field are its bottom and
// top halo planes (sy rows each) followed by its south halo rows (Hy per interior level); grid.y = field (wave-uniform table reads).
// Source and destination rows of a chunk have the same column offset, so the plain form (16-B aligned rows: fields on the 16-B grid,
// sx * sizeof(T) a multiple of 16 -- Float64 always, Float32 with Nx + 2 Hx = 0 mod 4) moves aligned 16-B vectors, and the GEN form
// (the project's name for element-aligned 16-B accesses, tpg_zipper_kernels.hpp) serves every other geometry: Float32 rows of
// Nx + 2 Hx = 2 mod 4 elements (3610 at the reference's model halo (5, 5, 5)) and element-aligned bases.  In the GEN form the last chunk of
// a row is moved back to end at the row's end and overlaps its neighbour: both write the same values (no source is written here).
#include "tpg_launch.hpp"

namespace {

struct BoundedTable {
    void* ptr[TPG_MAX_FIELDS];
    int sides[TPG_MAX_FIELDS];       // TPG_SIDE_* bits, already cleared where the geometry has no halo on that side
};

struct BoundedArgs {
    int sx, sy, Nz, Hy, Hz;
    int cpr;                         // chunks per row
    long long plane;                 // sx * sy
};

template <typename T, int W, bool GEN>
__global__ __launch_bounds__(256) void k_bounded_mirror(BoundedTable t, BoundedArgs a)
{
    typedef typename Vec<T, W>::aligned_t vec_t;
    typedef typename Vec<T, W>::loose_t lvec_t;
    typedef typename std::conditional<GEN, lvec_t, vec_t>::type cvec_t;
    const int f = blockIdx.y;
    const int sides = t.sides[f];
    const bool south = (sides & TPG_SIDE_SOUTH) != 0;
    const int nb = (sides & TPG_SIDE_BOTTOM) ? a.Hz : 0;
    const int zrows = (nb + ((sides & TPG_SIDE_TOP) ? a.Hz : 0)) * a.sy;
    const int rows = zrows + (south ? a.Nz * a.Hy : 0);
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= rows * a.cpr) return;
    const int r = item / a.cpr;
    const int ch = item - r * a.cpr;
    int pd, ps, jd, js;                                            // destination / source plane and row (0-based parent indices)
    if (r < zrows) {
        const int l = r / a.sy;                                    // halo level slot: bottom k = l+1, then top k = l-nb+1
        jd = r - l * a.sy;
        js = (south && jd < a.Hy) ? 2 * a.Hy - 1 - jd : jd;        // corner: c[i, 1-j, 1-k] = c[i, j, k]
        if (l < nb) { pd = a.Hz - 1 - l; ps = a.Hz + l; }
        else        { const int k = l - nb; pd = a.Hz + a.Nz + k; ps = a.Hz + a.Nz - 1 - k; }
    } else {
        const int q = r - zrows;
        const int k = q / a.Hy;                                    // interior level k+1
        jd = q - k * a.Hy;                                         // halo row 1-j with j = Hy - jd
        js = 2 * a.Hy - 1 - jd;
        pd = ps = a.Hz + k;
    }
    const int e0 = GEN ? min(ch * W, a.sx - W) : ch * W;
    T* c = static_cast<T*>(t.ptr[f]);
    const cvec_t v = *reinterpret_cast<const cvec_t*>(c + a.plane * ps + (long long)a.sx * js + e0);
    *reinterpret_cast<cvec_t*>(c + a.plane * pd + (long long)a.sx * jd + e0) = v;
}

}  // namespace

extern "C" {

int tpg_fill_bounded_halos(void* const fields[], int nfields, const uint8_t sides[],
                           int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc) return rc;
    if (!sides) { tpg::set_error("null sides table"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    const int all = TPG_SIDE_SOUTH | TPG_SIDE_BOTTOM | TPG_SIDE_TOP;
    int any = 0;
    for (int f = 0; f < nfields; ++f) {
        if (sides[f] & ~all) { tpg::set_error("field %d: sides = %d has bits other than TPG_SIDE_SOUTH | TPG_SIDE_BOTTOM | TPG_SIDE_TOP", f, (int)sides[f]); return TPG_ERR_INVALID_ARGUMENT; }
        if ((uintptr_t)fields[f] % esz) { tpg::set_error("field %d: pointer not aligned to its element type", f); return TPG_ERR_INVALID_ARGUMENT; }
        any |= sides[f];
    }
    // the mirror's sources must be interior rows / levels that the horizontal fill does not write (the zipper writes row Ny)
    if ((any & TPG_SIDE_SOUTH) && Ny <= Hy) {
        tpg::set_error("south no-flux mirror needs Ny > Hy (Ny = %d, Hy = %d)", Ny, Hy);
        return TPG_ERR_UNSUPPORTED;
    }
    if ((any & (TPG_SIDE_BOTTOM | TPG_SIDE_TOP)) && Nz < Hz) {
        tpg::set_error("bottom / top no-flux mirror needs Nz >= Hz (Nz = %d, Hz = %d)", Nz, Hz);
        return TPG_ERR_UNSUPPORTED;
    }
    // sides without a halo are no-ops
    const int keep = (Hy > 0 ? TPG_SIDE_SOUTH : 0) | (Hz > 0 ? TPG_SIDE_BOTTOM | TPG_SIDE_TOP : 0);
    if (!(any & keep)) return TPG_OK;
    Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    // plain 16-B chunks where every row starts on the 16-B grid, element-aligned 16-B (or, for rows shorter than 16 B, 8-B) chunks otherwise
    const int WMAX = (int)(16 / esz);
    const bool plain = rows_on_16B_grid((size_t)g.sx * esz, fields, nfields);
    const int W = plain || g.sx >= WMAX ? WMAX : 2;
    BoundedArgs a{ g.sx, g.sy, Nz, Hy, Hz, plain ? g.sx / W : (g.sx + W - 1) / W, g.plane };
    const long long max_rows = 2ll * Hz * g.sy + (long long)Nz * Hy;
    if (max_rows * a.cpr >= (1ll << 31) - 256) {
        tpg::set_error("bounded halos too large for 32-bit work-item indexing");
        return TPG_ERR_UNSUPPORTED;
    }
    hipStream_t s = tpg::as_stream(stream);
    return for_each_batch(nfields, [&](int f0, int n) {
        BoundedTable t;
        long long rows = 0;
        for (int f = 0; f < n; ++f) {
            t.ptr[f] = fields[f0 + f];
            t.sides[f] = sides[f0 + f] & keep;
            const long long rf = ((t.sides[f] & TPG_SIDE_BOTTOM) ? (long long)Hz * g.sy : 0) + ((t.sides[f] & TPG_SIDE_TOP) ? (long long)Hz * g.sy : 0)
                               + ((t.sides[f] & TPG_SIDE_SOUTH) ? (long long)Nz * Hy : 0);
            rows = rf > rows ? rf : rows;
        }
        if (rows == 0) return (int)TPG_OK;
        dim3 grid((unsigned)((rows * a.cpr + 255) / 256), (unsigned)n);
        dispatch_ft(ft, [&](auto ty) {
            dispatch_chunk<decltype(ty)>(W, !plain, [&](auto w, auto gen) {
                hipLaunchKernelGGL((k_bounded_mirror<decltype(ty), decltype(w)::value, decltype(gen)::value>), grid, dim3(256), 0, s, t, a);
            });
        });
        return tpg::launch_status("k_bounded_mirror");
    });
}

}  // extern "C"
