// tpg_zipper.hip -- north-seam Zipper halo fill (index reversal + vector sign flip) for gfx950,
// plus the periodic-x pass and the latitude-band pack/unpack kernels that sit either side of it.
//
// Replaces fold_north_{center_center,face_center,center_face,face_face}!
// (src/zipper_boundary_condition.jl:70-138) as invoked per (i,k) by _fill_north_halo! (:146-155).
//
// HBM-bound integer/index work, no MFMA.  Design:
//  * one launch folds a whole BATCH of fields (pointer table in the kernarg segment), all levels;
//  * a work item is one 16-byte chunk (2 doubles / 4 floats) of one destination row: rows
//    Ny+1..Ny+Hy, plus the upper half of row Ny for y-Center fields (the row-Ny substitution);
//  * consecutive lanes own consecutive destination chunks (ascending, 16-B aligned stores) and
//    read the mirrored source chunk (descending addresses, one contiguous 1 KiB window per wave),
//    reverse it in registers and multiply by the sign;
//  * x-Face rows mirror about an odd offset (i' = Nx - i + 2): their source windows are 8-B (f64)
//    / 4-B (f32) off 16-B alignment, read with dword-aligned wide loads;
//  * a 1-D grid of 256-thread blocks, grid-stride free (one item per thread), 64-bit element
//    offsets, 32-bit item indices.
// Geometries whose rows do not split into 16-B aligned chunks (odd Hx -- the reference's model halo (5, 5, 5) --, Float32 with Nx = 2 mod 4,
// 16-B-misaligned base pointers) run the same kernels in their GEN form: the same chunks, stored element-aligned (tpg_zipper_kernels.hpp).
// Which kernel a call gets, and how it is launched, is host code: tpg_launch.hpp.
#include "tpg_launch.hpp"

namespace tpg { thread_local hipEvent_t ev_start = nullptr, ev_stop = nullptr; }

namespace {

// one validated call: what the passes and the launch strategies of tpg_fill_halo_regions work from
struct FillCall { void* const* fields; int nfields; const int8_t *xloc, *yloc; const int32_t* sign; Geom g; int ft; hipStream_t s; };

int zipper_levels(const FillCall& c, int kstart, int kcount)
{
    return for_each_batch(c.nfields, [&](int f0, int n) {
        return dispatch_ft(c.ft, [&](auto ty) { return zipper_batch<decltype(ty)>(c.fields + f0, n, c.xloc + f0, c.yloc + f0, c.sign + f0, c.g, kstart, kcount, c.s); });
    });
}

int periodic_x(const FillCall& c)
{
    const Geom& g = c.g;
    if (g.Hx == 0) return TPG_OK;
    return for_each_batch(c.nfields, [&](int f0, int n) {
        PtrTable pt;
        for (int f = 0; f < n; ++f) pt.ptr[f] = c.fields[f0 + f];
        PerArgs a{ g.Nx, g.Hx, g.sx, (long long)g.sy * (g.Nz + 2 * g.Hz), n };
        const int epc = c.ft == TPG_F64 ? 2 : 4;
        if (g.Hx % epc == 0 && g.Nx % epc == 0 && rows_on_16B_grid(0, pt.ptr, n)) {
            const int cpr = g.Hx / epc;
            dim3 gridv((unsigned)((a.nrows * cpr + 255) / 256), (unsigned)n);
            TPG_LAUNCH(k_periodic_x_vec<u32x4>, gridv, dim3(256), c.s, pt, a, cpr, epc);
        } else {
            dim3 grid((unsigned)((a.nrows * g.Hx * n + 255) / 256));
            dispatch_ft(c.ft, [&](auto ty) { TPG_LAUNCH(k_periodic_x<decltype(ty)>, grid, dim3(256), c.s, pt, a); });
        }
        return tpg::launch_status("k_periodic_x");
    });
}

// the three launch strategies of tpg_fill_halo_regions (north side = zipper) return a status, or:
constexpr int NOT_APPLICABLE = 1 << 30;                        // "this strategy does not serve the call"

// the conditions the one-launch forms share: halos on both axes and folds / wraps that read wholly inside the interior
bool one_launch_geometry(const Geom& g) { return g.Hx > 0 && g.Hy > 0 && g.Nx >= 2 * g.Hx + 2 && g.Ny >= 2 * g.Hy + 2; }

// small fields: one fused launch (k_fill_fused_vec / k_fill_fused); TPG_FILL_FUSED=0 never, =1 whenever the geometry allows
int fill_fused(const FillCall& c)
{
    const Geom& g = c.g;
    const int mode = tpg::config().fill_fused;
    if (mode == 0 || !one_launch_geometry(g)) return NOT_APPLICABLE;
    const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, Hx = g.Hx, Hy = g.Hy, Hz = g.Hz;
    const long long per_level = (long long)(Hy + 1) * (Nx + 2 * Hx) + 2ll * Hx * (Ny + Hy - 1);
    const long long items = per_level * (Nz + 2 * Hz);
    if (!(items < (1ll << 31) && (mode >= 1 || items * c.nfields <= (1ll << 20)))) return NOT_APPLICABLE;
    return for_each_batch(c.nfields, [&](int f0, int n) {
        FieldTable t;
        fill_field_table(t, c.fields + f0, c.xloc + f0, c.yloc + f0, c.sign + f0, n);
        // chunk items (plain or GEN: chunk_plan); TPG_FILL_FUSED=2 (test library) forces the one-thread-per-cell form k_fill_fused
        dispatch_ft(c.ft, [&](auto ty) {
            typedef decltype(ty) T;
            if (mode != 2) {
                const ChunkPlan cp = chunk_plan<T>(g, t.ptr, n);
                const int W = cp.W, r = cp.gen ? Hx % W : 0;
                FusedVecArgs v{ Nx, Ny, Hx, Hy, Hz, Nz, g.sx, (long long)g.sx * g.sy, cp.gen ? 2 * (Hx / W) + Nx / W : g.sx / W,
                                cp.gen ? Hx : 2 * Hx / W, 0, 0, r, (Hy + 1) * 2 * r };
                v.itemsA = (Hy + 1) * v.cpr;
                v.per_level = v.itemsA + v.itemsS + (Ny + Hy - 1) * v.hc;
                dim3 gridv((unsigned)(((long long)v.per_level * (Nz + 2 * Hz) + 255) / 256), (unsigned)n);
                fused_vec_launch<T>(gridv, c.s, t, v, cp);
            } else {
                FusedArgs a{ Nx, Ny, Hx, Hy, Hz, Nz, g.sx, g.sy, (long long)g.sx * g.sy, (int)per_level };
                dim3 grid((unsigned)((items + 255) / 256), (unsigned)n);
                TPG_LAUNCH(k_fill_fused<T>, grid, dim3(256), c.s, t, a);
            }
        });
        return tpg::launch_status("k_fill_fused");
    });
}

// large fields: zipper (with its corner cells) + periodic x merged into one launch (plain or GEN: chunk_plan); TPG_FILL_MERGED=0 never
int fill_merged(const FillCall& c)
{
    const Geom& g = c.g;
    if (tpg::config().fill_merged == 0 || !one_launch_geometry(g) || g.Hy > 8 || (long long)g.Nz * g.sx >= (1ll << 31) - 256) return NOT_APPLICABLE;
    return dispatch_ft(c.ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, c.fields, c.nfields);            // one plan for the whole call (all batches)
        const int Nx = g.Nx, Nz = g.Nz, Hx = g.Hx, Hy = g.Hy, Hz = g.Hz, W = cp.W, r = cp.gen ? Hx % W : 0;
        MergedArgs a{ Nx, g.Ny, Hx, Hy, Hz, Nz, g.sx, g.sy, g.plane, cp.gen ? 2 * (Hx / W) + Nx / W : g.sx / W, cp.gen ? Hx : Hx / W, 0,
                      (long long)g.sy * (Nz + 2 * Hz), r, (unsigned)(((long long)Nz * 2 * r + 255) / 256) };
        a.blocksA = (unsigned)(((long long)Nz * a.cprA + 255) / 256);
        return for_each_batch(c.nfields, [&](int f0, int n) {
            FieldTable t;
            fill_field_table(t, c.fields + f0, c.xloc + f0, c.yloc + f0, c.sign + f0, n);
            return merged_batch<T>(t, a, n, Hy, cp, c.s);
        });
    });
}

// every other geometry (Hy = 0, Hy > 8, Nx < 2 Hx + 2, ...): the fold over the interior levels, then periodic x
int fill_two_launch(const FillCall& c) { const int rc = zipper_levels(c, 1, c.g.Nz); return rc ? rc : periodic_x(c); }

}  // namespace

extern "C" {

int tpg_zipper_fill(void* const fields[], int nfields, const int8_t xloc[], const int8_t yloc[],
                    const int32_t sign[], int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                    int kstart, int kcount, int ft, void* stream)
{
    int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc || (rc = check_locations(xloc, yloc, sign, nfields))) return rc;
    if (kcount < 0 || kstart < 1 - Hz || kstart + kcount - 1 > Nz + Hz) {
        tpg::set_error("level range %d:%d outside %d:%d", kstart, kstart + kcount - 1, 1 - Hz, Nz + Hz);
        return TPG_ERR_INVALID_ARGUMENT;
    }
    // Hy = 0 leaves no halo rows to fold, but the row-Ny substitution of the y-Center folds is outside the
    // j loop of the reference (zipper_boundary_condition.jl:102,135) and still applies
    if (kcount == 0) return TPG_OK;
    return zipper_levels({ fields, nfields, xloc, yloc, sign, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft, tpg::as_stream(stream) }, kstart, kcount);
}

int tpg_zipper_fill_timed(void* const fields[], int nfields, const int8_t xloc[], const int8_t yloc[],
                          const int32_t sign[], int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                          int kstart, int kcount, int ft, void* stream, void* start_event, void* stop_event)
{
    if (nfields > TPG_MAX_FIELDS) { tpg::set_error("timed launch: at most %d fields (one kernel)", TPG_MAX_FIELDS); return TPG_ERR_UNSUPPORTED; }
    TimedScope timed(start_event, stop_event);
    return tpg_zipper_fill(fields, nfields, xloc, yloc, sign, Nx, Ny, Nz, Hx, Hy, Hz, kstart, kcount, ft, stream);
}

int tpg_event_create(void** event)
{
    if (!event) { tpg::set_error("null event pointer"); return TPG_ERR_INVALID_ARGUMENT; }
    hipEvent_t e;
    // timing-only events: no system-scope fence when they complete (a default event attached to a launch turns the
    // kernel's end-of-dispatch release into a system-scope one, which lands inside the measured interval)
    int rc = tpg::hip_status(hipEventCreateWithFlags(&e, hipEventDisableSystemFence), "hipEventCreateWithFlags");
    *event = rc ? nullptr : e;
    return rc;
}

int tpg_event_destroy(void* event)
{
    return event ? tpg::hip_status(hipEventDestroy(static_cast<hipEvent_t>(event)), "hipEventDestroy") : TPG_OK;
}

int tpg_event_elapsed_ms(void* start_event, void* stop_event, float* ms)
{
    if (!start_event || !stop_event || !ms) { tpg::set_error("null event"); return TPG_ERR_INVALID_ARGUMENT; }
    int rc = tpg::hip_status(hipEventSynchronize(static_cast<hipEvent_t>(stop_event)), "hipEventSynchronize");
    if (rc) return rc;
    return tpg::hip_status(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start_event), static_cast<hipEvent_t>(stop_event)), "hipEventElapsedTime");
}

int tpg_periodic_x_fill(void* const fields[], int nfields, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                        int ft, void* stream)
{
    if (int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    return periodic_x({ fields, nfields, nullptr, nullptr, nullptr, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft, tpg::as_stream(stream) });
}

// fill_halo_regions! of one set of fields: the arguments are validated once, here (the location tables only where the north side is
// the zipper -- they may be NULL otherwise); then the first launch strategy that serves the geometry runs
int tpg_fill_halo_regions(void* const fields[], int nfields, const int8_t xloc[], const int8_t yloc[],
                          const int32_t sign[], int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                          int north_is_zipper, int ft, void* stream)
{
    int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft);
    if (rc) return rc;
    const FillCall c{ fields, nfields, xloc, yloc, sign, tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz), ft, tpg::as_stream(stream) };
    if (!north_is_zipper) return periodic_x(c);
    if ((rc = check_locations(xloc, yloc, sign, nfields))) return rc;
    if ((rc = fill_fused(c)) != NOT_APPLICABLE) return rc;
    if ((rc = fill_merged(c)) != NOT_APPLICABLE) return rc;
    return fill_two_launch(c);
}

int tpg_fill_halo_regions_timed(void* const fields[], int nfields, const int8_t xloc[], const int8_t yloc[],
                                const int32_t sign[], int Nx, int Ny, int Nz, int Hx, int Hy, int Hz,
                                int north_is_zipper, int ft, void* stream, void* start_event, void* stop_event)
{
    if (nfields > TPG_MAX_FIELDS) { tpg::set_error("timed launch: at most %d fields (one batch)", TPG_MAX_FIELDS); return TPG_ERR_UNSUPPORTED; }
    TimedScope timed(start_event, stop_event);
    return tpg_fill_halo_regions(fields, nfields, xloc, yloc, sign, Nx, Ny, Nz, Hx, Hy, Hz, north_is_zipper, ft, stream);
}

size_t tpg_y_halo_buffer_elems(int nfields, int Nx, int Nz, int Hx, int Hy, int Hz)
{
    if (nfields < 0 || Nx < 0 || Nz < 0 || Hx < 0 || Hy < 0 || Hz < 0) return 0;
    return (size_t)nfields * (size_t)(Nx + 2 * Hx) * (size_t)Hy * (size_t)(Nz + 2 * Hz);
}

static int pack_common(void* const fields[], int nfields, void* buffer, int side, bool pack,
                       int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = check_call(fields, nfields, Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (!buffer) { tpg::set_error("null message buffer"); return TPG_ERR_INVALID_ARGUMENT; }
    if (side != 0 && side != 1) { tpg::set_error("side must be 0 (south) or 1 (north)"); return TPG_ERR_INVALID_ARGUMENT; }
    if (nfields > TPG_MAX_FIELDS) { tpg::set_error("at most %d fields per message", TPG_MAX_FIELDS); return TPG_ERR_UNSUPPORTED; }
    if (Hy == 0) return TPG_OK;
    Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    // 0-based parent row of the slab: pack reads interior rows next to the side, unpack writes halo rows
    int row0 = pack ? (side == 0 ? Hy : Ny) : (side == 0 ? 0 : Ny + Hy);
    const size_t esz = ft == TPG_F64 ? 8 : 4;
    // 16-B chunks of the rows when every row start, the message buffer and every field base sit on the 16-B grid (Float64 with aligned
    // bases: always -- sx is even); otherwise 16-B chunks of the contiguous Hy x sx slabs through element-aligned accesses (k_pack_loose):
    // Float32 rows with sx = 2 mod 4 -- e.g. Nx = 3600 at the reference's model halo 5 -- or bases off the grid
    PtrTable pt;
    for (int f = 0; f < nfields; ++f) pt.ptr[f] = fields[f];
    const bool vec = rows_on_16B_grid((size_t)g.sx * esz, fields, nfields, buffer);
    const int W = (int)(16 / esz);
    PackArgs a{ g.sx, g.sy, Nz + 2 * Hz, Hy, row0, g.plane, nfields, vec ? W : 1 };
    long long total = vec ? (long long)nfields * a.nlev * Hy * g.sx / W : (long long)nfields * a.nlev * ((Hy * g.sx + W - 1) / W);
    dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = tpg::as_stream(stream);
    auto launch = [&](auto packing) {
        constexpr bool PACK = decltype(packing)::value;
        if (vec) hipLaunchKernelGGL((k_pack<u32x4, PACK>), grid, dim3(256), 0, s, pt, static_cast<u32x4*>(buffer), a);
        else dispatch_ft(ft, [&](auto ty) {
            hipLaunchKernelGGL((k_pack_loose<decltype(ty), 16 / (int)sizeof(ty), PACK>), grid, dim3(256), 0, s, pt, static_cast<decltype(ty)*>(buffer), a);
        });
    };
    if (pack) launch(std::true_type{}); else launch(std::false_type{});
    return tpg::launch_status("k_pack");
}

int tpg_pack_y_halo(void* const fields[], int nfields, void* buffer, int side,
                    int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    return pack_common(fields, nfields, buffer, side, true, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream);
}

int tpg_unpack_y_halo(void* const fields[], int nfields, const void* buffer, int side,
                      int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    return pack_common(fields, nfields, const_cast<void*>(buffer), side, false, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream);
}

}  // extern "C"

