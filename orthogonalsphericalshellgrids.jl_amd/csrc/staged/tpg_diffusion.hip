// tpg_diffusion.hip -- the explicit diffusive tendency of a hydrostatic model with its top and bottom boundary fluxes, for gfx950
// (tpg_diffusive_tendency): horizontal and vertical down-gradient fluxes of up to TPG_MAX_FIELDS fields at one horizontal location, the
// fluxes through the faces 1 (or the lowest wet cell's bottom face) and Nz + 1 from planes, and the faces between wet and dry cells closed --
// the first conditional flux in the tree.  ADDed to G after the advection and hydrostatic calls and before AB2.
// [recalled: Oceananigans' diffusive_flux_x/y/z, div_dot_q, apply_z_bcs!, conditional_flux with immersed_peripheral_node; parity unpinned,
// like every operator here]
//
// THE RULE is written out once, in tripolar_hip_diffusion.h beside this file.  Evaluated in the field type T with no contraction; every
// operation is one correctly rounded IEEE operation.
//
// HBM-bound, of the family of k_tracer_advection (tpg_advection.hip): a work item is ONE chunk of W interior columns x JT rows and walks ALL
// levels upwards, for TG fields that share the metrics, the diffusivities, the counts and the bottom height (grid.y counts the field groups).
// A call splits its fields greedily into groups of 4 (without the horizontal group), then of 2, then single ones (tracer_groups), one launch
// per group size.
// Once per column the item loads its cells of the metric planes, the bottom heights of its columns and of the cells west, east, south and
// north of them, the count values and the bottom flux planes; the top flux planes at the last level.  It carries from level to level, per
// field, Fz at the level's bottom face and the c rows of the level (which are "the level below" of the next): each c plane is fetched once
// for the vertical direction.  Under the lowest wet cell the carried Fz IS the bottom flux, handed upwards unchanged, so it takes no
// registers of its own.
// Per level: dz_c[k], dz_f and a profile kappa of the top face and z_centers[k] (wave-uniform), a FIELD kappa chunk per row, and per field the
// JT rows of c one level up and -- HORIZ -- the row south and the row north of the tile and one element west and east of each row at this
// level, and in ADD mode the rows of G.  No load depends on the previous level: the loads of the next LA levels are issued before the
// current level's arithmetic (a ring of register slots).  The closed-face test is one compare per neighbour and level, no branch: without
// a bottom height the heights are -inf against the constant 0.
// Items are numbered (row tile, chunk) with the chunk fastest, 256 to a block.  A single field with the horizontal group has tiles of two
// rows: rows of the last tile past the interior compute on the row offsets clamped onto row Ny + 1 (inside the north halo, Hy >= 1) and
// store nothing.  Every other form has one row per item; a call without the horizontal group reads the own column only.
// Compile-time forms: the element type, the chunk form (W, GEN), HORIZ and the fields per item; everything else -- the vertical group, ADD,
// the mask, the closure, the kappa form, the flux planes by null test -- is a wave-uniform run-time switch (profiles/diffusion/).
//
// 16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned otherwise: chunk_plan's plain / GEN split over
// all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing allocated, no host wait.
#include "tpg_operator.hpp"
#include "tpg_tracer_tendency.hpp"
#include "tripolar_hip_diffusion.h"
#include <cmath>
#include <limits>

// compile-time switches of profiles/diffusion/ (make -C staged DIFFUSION_TAG=_jt1 DIFFUSION_FLAGS=-DTPG_DIFF_JT=1, -DTPG_DIFF_TG=2,
// -DTPG_DIFF_LOOKAHEAD=1, -DTPG_DIFF_NT=0)
#ifndef TPG_DIFF_TG
#define TPG_DIFF_TG 4
#endif
#ifndef TPG_DIFF_JT
#define TPG_DIFF_JT 2
#endif
#ifndef TPG_DIFF_LOOKAHEAD
#define TPG_DIFF_LOOKAHEAD 2
#endif
#ifndef TPG_DIFF_NT
#define TPG_DIFF_NT 1
#endif

namespace {

// The forms that exist, chosen by the compiler's register and spill figures (profiles/diffusion/resources.json: no scratch and no vector-register
// spill in any of them).  Without the horizontal group a work item takes up to 4 fields on one row.  With it a group of 4 spills in every
// shape tried and a group of 2 on two rows spills in Float64, so the fields go in groups of 2 on one row, and a single field takes two rows.
constexpr int GROUP = TPG_DIFF_TG;         // the largest group of fields a work item takes without the horizontal group: 4, 2 or 1
constexpr int GROUP_H = GROUP < 2 ? GROUP : 2;                     // ... and with it
// rows per work item
template <bool HORIZ, int TG> constexpr int ROWS = HORIZ && TG == 1 ? TPG_DIFF_JT : 1;
// levels whose loads are in flight ahead of the arithmetic
template <bool HORIZ, int TG> constexpr int LOOKAHEAD = HORIZ || TG >= 4 ? 1 : TPG_DIFF_LOOKAHEAD;
constexpr bool NT = TPG_DIFF_NT;           // G goes out in streaming stores

struct DiffPtrs {
    const void* c[TPG_MAX_FIELDS];
    void* G[TPG_MAX_FIELDS];
    const void* top[TPG_MAX_FIELDS];       // null: no flux through the face Nz + 1 of the field
    const void* bottom[TPG_MAX_FIELDS];    // null: no flux through the bottom face of the field's lowest wet cell
    const void *dx_fc, *dy_fc, *dx_cf, *dy_cf, *az, *dz_c, *dz_f;
    const void* kappa;                     // PROFILE: Nz + 1 values; FIELD: a padded parent; CONSTANT: null
    const void *h, *zc;                    // the bottom height and the z centres, or null: no face is closed
    const int32_t* counts;                 // null, or an Ny x Nx plane
};

struct DiffArgs {
    int Nx, Ny, Nz, sx;
    int q0;                                // the launch's first field
    int cpr;                               // chunks per interior row
    int items;                             // row tiles x cpr
    int vertical;                          // the vertical group is present
    int interior;                          // ... with the interior faces: terms & TPG_DIFFUSION_VERTICAL
    int add;                               // TPG_DIFFUSION_ADD
    int form;                              // kappa_z_form
    int wall;                              // south_is_wall, with a bottom height
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double kh, kz, value;                  // T values held in doubles: kappa_h, the constant kappa_z, the mask value
};

template <typename T, int W, bool GEN, bool HORIZ, int TG>
__global__ __launch_bounds__(256) void k_diffusive_tendency(DiffPtrs p, DiffArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    constexpr int JT = ROWS<HORIZ, TG>;
    constexpr int LA = LOOKAHEAD<HORIZ, TG>;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int e0 = (item - tile * a.cpr) * W;                      // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const int q0 = a.q0 + blockIdx.y * TG;                         // first field of the group
    const int Nz = a.Nz;
    const bool closure = HORIZ && p.h != nullptr, field_kappa = a.form == TPG_DIFFUSION_KAPPA_FIELD;
    auto chunk = [](const T* q) { return *reinterpret_cast<const cvec_t*>(q); };

    // row offsets inside a plane: the tile's rows and the row to the north of the last, clamped onto the row north of the last interior one
    // (row nr <= Ny of the tile: inside the interior or the first north halo row, Hy >= 1); with one row per item nothing is clamped
    int ro[JT + 1];
#pragma unroll
    for (int r = 0; r <= JT; ++r) ro[r] = a.sx * min(r, nr);
    // what belongs to a row alone -- az, a FIELD kappa, the flux planes, G, the west and east elements -- is read inside the interior only: a
    // row past the interior takes the tile's first row there
    int rq[JT];
#pragma unroll
    for (int r = 0; r < JT; ++r) rq[r] = r < nr ? ro[r] : 0;

    // the tile's metrics, heights and counts, once
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    const T* az = static_cast<const T*>(p.az) + m0;
    T azr[JT][W];
    int m[JT][W];                                                  // masked levels (0-based k < m): the first wet cell is m
    T kdy[JT][W + 1], rdx[JT][W + 1];                              // HORIZ: dy_fc and dx_fc at the faces i .. i + W of each row
    T kdx[JT + 1][W], rdy[JT + 1][W];                              // HORIZ: dx_cf and dy_cf at the faces j0 .. j0 + JT
    T hc[JT + 2][W], hw[JT], he[JT];                               // HORIZ: h of the rows j0 - 1 .. j0 + JT, and west and east of each row
    const T ninf = -std::numeric_limits<T>::infinity();
#pragma unroll
    for (int r = 0; r < JT; ++r) {
        const cvec_t z = chunk(az + rq[r]);
#pragma unroll
        for (int e = 0; e < W; ++e) { azr[r][e] = z[e]; m[r][e] = 0; }
        if (p.counts) {                                            // a count plane has no halo: clamped onto the last interior row
            const Counts<W> n = *reinterpret_cast<const Counts<W>*>(p.counts + (long long)a.Nx * (j0 + min(r, nr - 1)) + e0);
#pragma unroll
            for (int e = 0; e < W; ++e) m[r][e] = min(max(n[e], 0), Nz);
        }
    }
    if constexpr (HORIZ) {
        const T* dyf = static_cast<const T*>(p.dy_fc) + m0;
        const T* dxf = static_cast<const T*>(p.dx_fc) + m0;
        const T* dxc = static_cast<const T*>(p.dx_cf) + m0;
        const T* dyc = static_cast<const T*>(p.dy_cf) + m0;
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            const cvec_t y = chunk(dyf + rq[r]), x = chunk(dxf + rq[r]);
            kdy[r][W] = dyf[rq[r] + W];                            // the face i + 1 of the chunk's last column
            rdx[r][W] = dxf[rq[r] + W];
#pragma unroll
            for (int e = 0; e < W; ++e) { kdy[r][e] = y[e]; rdx[r][e] = x[e]; }
        }
#pragma unroll
        for (int r = 0; r <= JT; ++r) {
            const cvec_t x = chunk(dxc + ro[r]), y = chunk(dyc + ro[r]);                       // rows j0 .. j0 + JT
#pragma unroll
            for (int e = 0; e < W; ++e) { kdx[r][e] = x[e]; rdy[r][e] = y[e]; }
        }
#pragma unroll
        for (int r = 0; r < JT + 2; ++r)
#pragma unroll
            for (int e = 0; e < W; ++e) hc[r][e] = ninf;
#pragma unroll
        for (int r = 0; r < JT; ++r) hw[r] = he[r] = ninf;
        if (closure) {
            const T* h = static_cast<const T*>(p.h) + m0;
            const cvec_t s = chunk(h - a.sx);
#pragma unroll
            for (int e = 0; e < W; ++e) hc[0][e] = s[e];
#pragma unroll
            for (int r = 0; r <= JT; ++r) {
                if (r < JT) { hw[r] = h[rq[r] - 1]; he[r] = h[rq[r] + W]; }
                const cvec_t x = chunk(h + ro[r]);
#pragma unroll
                for (int e = 0; e < W; ++e) hc[r + 1][e] = x[e];
            }
        }
    }
    const bool wall_s = closure && a.wall && j0 == 0;              // the cells south of the tile are inactive whatever h holds there

    const long long f0 = a.off3 + (long long)a.sx * j0 + e0;
    const T* dzc = static_cast<const T*>(p.dz_c);
    const T* dzf = static_cast<const T*>(p.dz_f);
    const T* zc = static_cast<const T*>(p.zc);
    const T* ktab = static_cast<const T*>(p.kappa);                                   // PROFILE
    const T* kfld = field_kappa ? static_cast<const T*>(p.kappa) + f0 : nullptr;      // FIELD: face k (0-based: under cell k) at plane Hz + k
    const T* c[TG];
    T* G[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        c[t] = static_cast<const T*>(p.c[q0 + t]) + f0;
        G[t] = static_cast<T*>(p.G[q0 + t]) + f0;
    }
    const T mv = (T)a.value, kh = (T)a.kh, kconst = (T)a.kz;

    struct Level {
        T d, df, kp, z;                                            // dz_c[k]; dz_f and kappa of the top face; z_centers[k]
        cvec_t kap[JT];                                            // FIELD: kappa at the top face
        cvec_t ca[TG][JT];                                         // c one level up
        cvec_t cs[TG], cn[TG];                                     // HORIZ: the rows south and north of the tile at this level
        T cw[TG][JT], ce[TG][JT];                                  // HORIZ: c one element west and east of each row at this level
        cvec_t g[TG][JT];                                          // ADD: G at this level
    };
    auto load = [&](Level& L, int k) {
        const int kt = min(k + 1, Nz - 1);                         // the top face (0-based: over cell k); the closed one clamped onto the last open one
        L.d = dzc[k];
        L.df = T(1);
        L.kp = kconst;
        L.z = T(0);
#pragma unroll
        for (int r = 0; r < JT; ++r) L.kap[r] = cvec_t{};         // read (and dropped by a select) where no face of kappa is loaded
        if (closure) L.z = zc[k];
        if (a.interior && Nz > 1) {                                // one level: no open face, nothing of kappa or dz_f is loaded
            L.df = dzf[kt];
            if (field_kappa) {
#pragma unroll
                for (int r = 0; r < JT; ++r) L.kap[r] = chunk(kfld + a.plane * kt + rq[r]);
            } else if (a.form == TPG_DIFFUSION_KAPPA_PROFILE) L.kp = ktab[kt];
        }
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            const T* ck = c[t] + a.plane * k;
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                L.ca[t][r] = chunk(c[t] + a.plane * kt + ro[r]);
                if constexpr (HORIZ) { L.cw[t][r] = ck[rq[r] - 1]; L.ce[t][r] = ck[rq[r] + W]; }
                if (a.add) L.g[t][r] = chunk(G[t] + a.plane * k + rq[r]);
            }
            if constexpr (HORIZ) { L.cs[t] = chunk(ck - a.sx); L.cn[t] = chunk(ck + ro[JT]); }
        }
    };

    // carried from level to level: the c rows of the level and Fz at its bottom face; under the lowest wet cell that is the bottom flux
    T cc[TG][JT][W], fzb[TG][JT][W];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const T* jb = static_cast<const T*>(p.bottom[q0 + t]);
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            const cvec_t c1 = chunk(c[t] + ro[r]);
            cvec_t b = cvec_t{};
            if (jb) b = chunk(jb + m0 + rq[r]);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                cc[t][r][e] = c1[e];
                fzb[t][r][e] = jb ? -(azr[r][e] * b[e]) : T(0);
            }
        }
    }

    Level ring[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) load(ring[s], min(s, Nz - 1));
    for (int k0 = 0; k0 < Nz; k0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int k = k0 + s;
            if (k >= Nz) break;
            const Level L = ring[s];
            if (k + LA < Nz) load(ring[s], k + LA);                // the loads of level k + LA go out before level k's arithmetic
            const T d = L.d, zk = L.z;
            const bool top = k == Nz - 1;
            // inactive cells of this level: the rows j0 - 1 .. j0 + JT, and west and east of each row
            bool ic[JT + 2][W], iw[JT], ie[JT];
            if constexpr (HORIZ) {
#pragma unroll
                for (int r = 0; r < JT + 2; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) ic[r][e] = zk <= hc[r][e];
#pragma unroll
                for (int e = 0; e < W; ++e) ic[0][e] = ic[0][e] || wall_s;
#pragma unroll
                for (int r = 0; r < JT; ++r) { iw[r] = zk <= hw[r]; ie[r] = zk <= he[r]; }
            }
            T fys[TG][W];                                          // Fy at the south face of the row: the previous row's north face
            if constexpr (HORIZ) {
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const T ay = kh * (kdx[0][e] * d);
                    const bool closed = ic[0][e] || ic[1][e];
#pragma unroll
                    for (int t = 0; t < TG; ++t) fys[t][e] = closed ? T(0) : ay * ((cc[t][0][e] - L.cs[t][e]) / rdy[0][e]);
                }
            }
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                T ax[W + 1], ay[W], akz[W], rV[W];
                bool cx_[W + 1], cy_[W];                           // closed faces: i .. i + W of the row; the row's north face
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    if constexpr (HORIZ) {
                        ax[e] = kh * (kdy[r][e] * d);
                        ay[e] = kh * (kdx[r + 1][e] * d);
                        cx_[e] = (e == 0 ? iw[r] : ic[r + 1][e - 1]) || ic[r + 1][e];
                        cy_[e] = ic[r + 1][e] || ic[r + 2][e];
                    }
                    akz[e] = (field_kappa ? L.kap[r][e] : L.kp) * azr[r][e];
                    rV[e] = T(1) / (azr[r][e] * d);
                }
                if constexpr (HORIZ) {
                    ax[W] = kh * (kdy[r][W] * d);
                    cx_[W] = ic[r + 1][W - 1] || ie[r];
                }
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    T cx[W + 2], cnr[W];                           // the row with its west and east neighbours; the row to the north
                    cvec_t jt = cvec_t{};
                    const T* jtp = static_cast<const T*>(p.top[q0 + t]);
                    if (a.vertical && top && jtp) jt = chunk(jtp + m0 + rq[r]);
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        cx[e + 1] = cc[t][r][e];
                        if constexpr (HORIZ) {
                            if (r + 1 < JT) cnr[e] = cc[t][(r + 1) % JT][e];
                            else cnr[e] = L.cn[t][e];
                        }
                    }
                    T fw = T(0);                                   // for e > 0 it is the fe of e - 1
                    if constexpr (HORIZ) {
                        cx[0] = L.cw[t][r];
                        cx[W + 1] = L.ce[t][r];
                        fw = cx_[0] ? T(0) : ax[0] * ((cx[1] - cx[0]) / rdx[r][0]);
                    }
                    cvec_t out;
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        T S = T(0);
                        if constexpr (HORIZ) {
                            const T fe = cx_[e + 1] ? T(0) : ax[e + 1] * ((cx[e + 2] - cx[e + 1]) / rdx[r][e + 1]);
                            const T fn = cy_[e] ? T(0) : ay[e] * ((cnr[e] - cx[e + 1]) / rdy[r + 1][e]);
                            S = (fe - fw) + (fn - fys[t][e]);
                            fw = fe;
                            fys[t][e] = fn;
                        }
                        if (a.vertical) {
                            const T open = a.interior ? akz[e] * ((L.ca[t][r][e] - cx[e + 1]) / L.df) : T(0);
                            const T ft_ = jtp ? -(azr[r][e] * jt[e]) : T(0);
                            // under the lowest wet cell the bottom flux is handed upwards unchanged
                            const T fzt = top ? ft_ : (k < m[r][e] ? fzb[t][r][e] : open);
                            const T vs = fzt - fzb[t][r][e];
                            fzb[t][r][e] = fzt;
                            if constexpr (HORIZ) S = S + vs;
                            else S = vs;
                        }
                        T g = rV[e] * S;
                        if (a.add) g = L.g[t][r][e] + g;
                        out[e] = k < m[r][e] ? mv : g;
                    }
                    if (r < nr) store_chunk<NT>(reinterpret_cast<cvec_t*>(G[t] + a.plane * k + a.sx * r), out);
                }
            }
#pragma unroll
            for (int t = 0; t < TG; ++t)
#pragma unroll
                for (int r = 0; r < JT; ++r)
#pragma unroll
                    for (int e = 0; e < W; ++e) cc[t][r][e] = L.ca[t][r][e];
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_diffusion_last_error(void) { return tpg_last_error(); }

int tpg_diffusive_tendency(const void* const* c, void* const* G, int nfields, int terms, int mode, double kappa_h, const void* kappa_z,
                           double kappa_z_value, int kappa_z_form, const void* const* top_flux, const void* const* bottom_flux,
                           const void* dx_fc, const void* dy_fc, const void* dx_cf, const void* dy_cf, const void* az, const void* dz_c,
                           const void* dz_f, const int32_t* counts, double mask_value, const void* bottom_height, const void* z_centers,
                           int south_is_wall, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    const int INVALID = TPG_ERR_INVALID_ARGUMENT, UNSUPPORTED = TPG_ERR_UNSUPPORTED;
    // 1. the geometry
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    // 2. the fields
    if (nfields < 1) { tpg::set_error("no fields (nfields = %d)", nfields); return INVALID; }
    if (nfields > TPG_MAX_FIELDS) { tpg::set_error("%d fields: at most TPG_MAX_FIELDS = %d in one call", nfields, TPG_MAX_FIELDS); return INVALID; }
    if (!c || !G) { tpg::set_error("null table of fields or of tendencies"); return INVALID; }
    for (int q = 0; q < nfields; ++q) {
        if (!c[q]) { tpg::set_error("null field %d", q); return INVALID; }
        if (!G[q]) { tpg::set_error("null G of field %d", q); return INVALID; }
    }
    // 3. the groups
    if (terms & ~(TPG_DIFFUSION_HORIZONTAL | TPG_DIFFUSION_VERTICAL)) {
        tpg::set_error("terms %d has bits that are not built (TPG_DIFFUSION_HORIZONTAL = 1 and TPG_DIFFUSION_VERTICAL = 2 are)", terms);
        return UNSUPPORTED;
    }
    const bool horizontal = terms & TPG_DIFFUSION_HORIZONTAL, interior = terms & TPG_DIFFUSION_VERTICAL;
    const bool vertical = interior || top_flux || bottom_flux;
    if (!horizontal && !vertical) { tpg::set_error("no group is present: terms = 0 and no table of top or bottom fluxes"); return INVALID; }
    // 4. the mode, then the form
    if (mode != TPG_DIFFUSION_ADD && mode != TPG_DIFFUSION_WRITE) {
        tpg::set_error("mode %d is not built (TPG_DIFFUSION_ADD = 0 and TPG_DIFFUSION_WRITE = 1 are)", mode);
        return UNSUPPORTED;
    }
    if (kappa_z_form != TPG_DIFFUSION_KAPPA_CONSTANT && kappa_z_form != TPG_DIFFUSION_KAPPA_PROFILE && kappa_z_form != TPG_DIFFUSION_KAPPA_FIELD) {
        tpg::set_error("kappa_z form %d is not built (TPG_DIFFUSION_KAPPA_CONSTANT = 0, TPG_DIFFUSION_KAPPA_PROFILE = 1 and "
                       "TPG_DIFFUSION_KAPPA_FIELD = 2 are)", kappa_z_form);
        return UNSUPPORTED;
    }
    // 5. the null combinations
    const bool constant = kappa_z_form == TPG_DIFFUSION_KAPPA_CONSTANT, field = kappa_z_form == TPG_DIFFUSION_KAPPA_FIELD;
    if (constant && kappa_z) { tpg::set_error("kappa_z given with TPG_DIFFUSION_KAPPA_CONSTANT: the diffusivity is kappa_z_value"); return INVALID; }
    if (!constant && !kappa_z) {
        tpg::set_error("null kappa_z with %s", field ? "TPG_DIFFUSION_KAPPA_FIELD" : "TPG_DIFFUSION_KAPPA_PROFILE");
        return INVALID;
    }
    if (!dz_c || !az) { tpg::set_error("null dz_c or az"); return INVALID; }
    if (interior && !dz_f) { tpg::set_error("null dz_f with TPG_DIFFUSION_VERTICAL"); return INVALID; }
    if (horizontal && (!dx_fc || !dy_fc || !dx_cf || !dy_cf)) {
        tpg::set_error("null dx_fc, dy_fc, dx_cf or dy_cf with TPG_DIFFUSION_HORIZONTAL");
        return INVALID;
    }
    if (bottom_height && !z_centers) { tpg::set_error("bottom_height without z_centers"); return INVALID; }
    // 6. the numbers
    if (horizontal && !std::isfinite(kappa_h)) { tpg::set_error("kappa_h is not finite"); return INVALID; }
    if (interior && constant && !std::isfinite(kappa_z_value)) { tpg::set_error("kappa_z_value is not finite"); return INVALID; }
    // 7. alignment
    const size_t esz = elem_size(ft);
    for (int q = 0; q < nfields; ++q)
        if (misaligned(esz, c[q])) { tpg::set_error("field %d: pointer not aligned to its element type", q); return INVALID; }
    for (int q = 0; q < nfields; ++q)
        if (misaligned(esz, G[q])) { tpg::set_error("G of field %d: pointer not aligned to its element type", q); return INVALID; }
    for (int q = 0; q < nfields; ++q)
        if (misaligned(esz, top_flux ? top_flux[q] : nullptr, bottom_flux ? bottom_flux[q] : nullptr)) {
            tpg::set_error("flux plane of field %d: pointer not aligned to its element type", q);
            return INVALID;
        }
    if (misaligned(esz, kappa_z, dx_fc, dy_fc, dx_cf, dy_cf, az, dz_c, dz_f, bottom_height, z_centers)) {
        tpg::set_error("kappa_z, a metric plane, dz_c, dz_f, bottom_height or z_centers pointer not aligned to its element type");
        return INVALID;
    }
    if (misaligned(4, counts)) { tpg::set_error("count plane pointer not aligned to int32"); return INVALID; }
    // 8. the overlaps: every G against every array the kernel reads through a neighbour's item or through another field's
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (Nz + 2 * Hz) * esz, pbytes = (unsigned long long)g.plane * esz;
    const unsigned long long kbytes = (unsigned long long)g.plane * (Nz + 1 + 2 * Hz) * esz;              // a FIELD kappa: one more level
    for (int q = 0; q < nfields; ++q) {
        auto hit = [&](const void* other, unsigned long long n) { return other && arrays_overlap(G[q], bytes, other, n); };
        for (int r = 0; r < nfields; ++r)
            if (hit(c[r], bytes)) {
                tpg::set_error("G of field %d overlaps field %d (every item reads cells while its neighbours write: not an in-place call)", q, r);
                return INVALID;
            }
        for (int r = 0; r < q; ++r)
            if (hit(G[r], bytes)) { tpg::set_error("G of field %d overlaps G of field %d", q, r); return INVALID; }
        if (field && hit(kappa_z, kbytes)) { tpg::set_error("G of field %d overlaps kappa_z", q); return INVALID; }
        for (int r = 0; r < nfields; ++r) {
            if (top_flux && hit(top_flux[r], pbytes)) { tpg::set_error("G of field %d overlaps the top flux plane of field %d", q, r); return INVALID; }
            if (bottom_flux && hit(bottom_flux[r], pbytes)) { tpg::set_error("G of field %d overlaps the bottom flux plane of field %d", q, r); return INVALID; }
        }
        if (hit(bottom_height, pbytes)) { tpg::set_error("G of field %d overlaps bottom_height", q); return INVALID; }
    }
    // 9. the stencil
    if (horizontal && (Hx < 1 || Hy < 1)) {
        tpg::set_error("the rule reads c[i-1..i+1, j, k], c[i, j-1..j+1, k] and the same cells of bottom_height: Hx >= 1 and Hy >= 1 needed with "
                       "TPG_DIFFUSION_HORIZONTAL (halo (%d,%d,%d))", Hx, Hy, Hz);
        return UNSUPPORTED;
    }
    // 10. the work items
    // (the plane check of 1. refuses every such geometry first: Nx * Ny < 2^31 there; kept for a change of either bound)
    if ((long long)Ny * (Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("diffusive tendency: too many work items for 32-bit indexing"); return UNSUPPORTED; }

    DiffPtrs p{};
    void* arrays[4 * TPG_MAX_FIELDS + 8];
    int na = 0;
    for (int q = 0; q < nfields; ++q) {
        p.c[q] = c[q]; p.G[q] = G[q];
        p.top[q] = top_flux ? top_flux[q] : nullptr;
        p.bottom[q] = bottom_flux ? bottom_flux[q] : nullptr;
        for (const void* x : { c[q], (const void*)G[q], p.top[q], p.bottom[q] })
            if (x) arrays[na++] = const_cast<void*>(x);
    }
    p.az = az; p.dz_c = dz_c; p.dz_f = dz_f; p.kappa = kappa_z; p.counts = counts;
    arrays[na++] = const_cast<void*>(az);
    if (field && interior) arrays[na++] = const_cast<void*>(kappa_z);
    if (horizontal) {
        p.dx_fc = dx_fc; p.dy_fc = dy_fc; p.dx_cf = dx_cf; p.dy_cf = dy_cf; p.h = bottom_height; p.zc = z_centers;
        for (const void* x : { dx_fc, dy_fc, dx_cf, dy_cf, bottom_height })
            if (x) arrays[na++] = const_cast<void*>(x);
    }
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, arrays, na);
        const int cpr = Nx / cp.W;
        DiffArgs a{ Nx, Ny, Nz, g.sx, 0, cpr, 0, vertical, interior, mode == TPG_DIFFUSION_ADD, kappa_z_form,
                    bottom_height && south_is_wall, g.plane, interior2(g), interior3(g), horizontal ? (double)(T)kappa_h : 0.0,
                    interior && constant ? (double)(T)kappa_z_value : 0.0, counts ? (double)(T)mask_value : 0.0 };
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            constexpr int W = decltype(cw)::value;
            constexpr bool GEN = decltype(gen)::value;
            auto launch = [&](auto horiz) {
                constexpr bool HORIZ = decltype(horiz)::value;
                tracer_groups<(HORIZ ? GROUP_H : GROUP)>(nfields, [&](auto tg, int q0, int n) {
                    constexpr int TG = decltype(tg)::value;
                    constexpr int JT = ROWS<HORIZ, TG>;
                    a.q0 = q0;
                    a.items = (Ny + JT - 1) / JT * cpr;
                    const unsigned blocks = (unsigned)((a.items + 255) / 256);
                    hipLaunchKernelGGL((k_diffusive_tendency<T, W, GEN, HORIZ, TG>), dim3(blocks, n), dim3(256), 0, st, p, a);
                });
            };
            if (horizontal) launch(std::true_type{});
            else            launch(std::false_type{});
        });
        return tpg::launch_status("k_diffusive_tendency");
    });
}

}  // extern "C"
