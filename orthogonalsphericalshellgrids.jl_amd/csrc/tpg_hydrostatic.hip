// tpg_hydrostatic.hip -- the Coriolis and the hydrostatic pressure-gradient tendencies of the horizontal velocities, accumulated into or written
// to Gu at (Face, Center, Center) and Gv at (Center, Face, Center), and the hydrostatic pressure anomaly at (Center, Center, Center), for gfx950
// (tpg_hydrostatic_tendencies): what a model with `coriolis = HydrostaticSphericalCoriolis()` and `buoyancy = BuoyancyTracer()` adds to the
// tendencies the advection calls leave, before the AB2 step of the velocities (tpg_ab2_step_velocities) consumes them.
// [recalled: Oceananigans' update_hydrostatic_pressure!, d/dx of pHY' and x_f_cross_U / y_f_cross_U of HydrostaticSphericalCoriolis with the
// EnstrophyConserving and EnergyConserving schemes; parity unpinned, like every operator here]
//
// THE RULE is written out once, in include/tripolar_hip_hydrostatic.h.  Evaluated in the field type T with no contraction; every operation
// is one correctly rounded IEEE operation.  Hx, Hy, Hz >= 1; only interior cells of Gu, Gv and p_out are written.
//
// ONE launch for everything, of the family of k_momentum_advection (tpg_momentum.hip) and k_w_from_continuity (tpg_continuity.hip): a work
// item is ONE chunk of W interior columns x JT rows.  It loads once the cells of the metric planes and of f_ff its nodes read and the count
// values, and walks ALL levels TOP-DOWN.  It carries from level to level PH of its own columns, of the column west of each of its rows and
// of the row south of the tile, and b one level up at the same cells: PH beside the tile is the same fixed sequence of operations on b
// loaded once more (an element per row and a chunk per tile), so the same bits.  With SHARE the column west comes from the neighbouring lane
// instead (__shfl_up) and only a lane whose neighbour is not in its wave or not in its row (the periodic seam) loads and carries it.  Per
// level: dz_f of the level's top face (wave-uniform), the rows of b, v, u the header lists and, in ADD mode, Gu and Gv at the nodes.  No
// load depends on the previous level: the loads of the next LOOKAHEAD levels are issued before the current level's arithmetic (a ring of
// register slots).  Items are numbered (row tile, chunk) with the chunk fastest, 256 to a block.  Rows of the last tile past the interior
// compute on the row offsets clamped onto row Ny + 1 (inside the north halo) and store nothing.
//
// The terms present are compile-time (COR: 0 none, 1 enstrophy-conserving, 2 energy-conserving; PRES); the mode, the mask and which outputs
// are given are wave-uniform run-time flags.  16-B chunks where rows and pointers sit on the 16-B grid, the same chunks element-aligned
// otherwise: chunk_plan's plain / GEN split over all the arrays passed.  Element offsets are 64-bit.  No atomics, no LDS, nothing
// allocated, no host wait.
#include "tpg_operator.hpp"
#include "../../include/tripolar_hip_hydrostatic.h"

// compile-time switches of the A/B in profiles/hydrostatic/ (make HYDROSTATIC_TAG=_jt4 HYDROSTATIC_FLAGS='-DTPG_HYD_JT=4 -DTPG_HYD_JT_F32=4', -DTPG_HYD_JT_F32=2,
// -DTPG_HYD_SHARE=1, -DTPG_HYD_LOOKAHEAD=2, -DTPG_HYD_WAVES=2 or -DTPG_HYD_NT=0).  What was measured at 3600 x 1800 x 75 and why these are the defaults:
// DESIGN.md 6, profiles/hydrostatic/.
#ifndef TPG_HYD_JT
#define TPG_HYD_JT 2
#endif
#ifndef TPG_HYD_JT_F32
#define TPG_HYD_JT_F32 1
#endif
#ifndef TPG_HYD_LOOKAHEAD
#define TPG_HYD_LOOKAHEAD 1
#endif
#ifndef TPG_HYD_SHARE
#define TPG_HYD_SHARE 0
#endif
#ifndef TPG_HYD_NT
#define TPG_HYD_NT 1
#endif
#ifndef TPG_HYD_WAVES
#define TPG_HYD_WAVES 1
#endif

namespace {

template <typename T> constexpr int ROWS = sizeof(T) == 8 ? TPG_HYD_JT : TPG_HYD_JT_F32;      // rows per work item (JT below)
constexpr int LOOKAHEAD = TPG_HYD_LOOKAHEAD;   // levels whose loads are in flight
constexpr bool SHARE = TPG_HYD_SHARE;          // PH west of a chunk from the neighbouring lane
constexpr bool NT = TPG_HYD_NT;                // Gu, Gv, p_out go out in streaming stores
constexpr int WAVES = TPG_HYD_WAVES;           // waves per SIMD the register allocation must leave room for (2: at most 256 VGPRs)

struct HydrostaticPtrs {
    const void *u, *v, *b;
    void *Gu, *Gv, *p;
    const void *f, *dxfc, *dyfc, *dxcf, *dycf, *dz;
    const int32_t *nfc, *ncf;
};

struct HydrostaticArgs {
    int Nx, Ny, Nz, sx;
    int cpr;                               // chunks per interior row
    int items;                             // row tiles x cpr
    long long plane;                       // sx * sy
    long long off2;                        // sx * Hy + Hx: the first interior cell of a padded plane
    long long off3;                        // plane * Hz + off2
    double value;                          // the mask value (a T value held in a double)
    int add, masked, hasG, hasP;           // mode == TPG_TENDENCY_ADD; count planes given; Gu and Gv given; p_out given
};

// Arrays of the tile are indexed [r + 1][c + 1] where a row r = -1 or a column c = -1 is read, [r][c] otherwise: r = -1 is the row south
// of the tile, r = JT the row north of it, c = -1 the column west of the chunk, c = W the column east of it.  Entries the rule does not
// read are never loaded and never used.
template <typename T, int W, bool GEN, int COR, bool PRES, int JT, int LA>
__global__ __launch_bounds__(256, WAVES) void k_hydrostatic_tendencies(HydrostaticPtrs p, HydrostaticArgs a)
{
    typedef Chunk<T, W, GEN> cvec_t;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.items) return;
    const int tile = item / a.cpr;
    const int ch = item - tile * a.cpr;
    const int e0 = ch * W;                                         // first interior column of the chunk (0-based)
    const int j0 = tile * JT;                                      // first interior row of the tile (0-based)
    const int nr = min(JT, a.Ny - j0);                             // rows of the tile inside the interior
    const T half = T(0.5);
    const bool hasG = a.hasG, add = a.add, masked = a.masked;
    // the column west of the chunk is this lane's own to load and carry, unless the lane west holds it: the same tile, the same wave
    const bool own_west = !(SHARE && (threadIdx.x & 63) > 0 && ch > 0);

    // row offsets inside a plane, rows -1 .. JT of the tile: the rows past the interior clamped onto the row north of the last interior one
    // (row nr <= Ny of the tile: inside the interior or the first north halo row, Hy >= 1)
    int ro[JT + 2];
#pragma unroll
    for (int r = -1; r <= JT; ++r) ro[r + 1] = a.sx * min(r, nr);
    auto chunk = [](const T* q) { return *reinterpret_cast<const cvec_t*>(q); };

    // the tile's metrics and f, once
    const long long m0 = a.off2 + (long long)a.sx * j0 + e0;
    T dxfc[JT][W], dycf[JT][W], dxcf[JT + 1][W + 1], dyfc[JT + 1][W + 1], f[JT + 1][W + 1];
    int mu[JT][W], mv[JT][W];
    if (hasG) {
        const T* dx = static_cast<const T*>(p.dxfc) + m0;
        const T* dy = static_cast<const T*>(p.dycf) + m0;
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            const cvec_t x = chunk(dx + ro[r + 1]), y = chunk(dy + ro[r + 1]);
#pragma unroll
            for (int e = 0; e < W; ++e) { dxfc[r][e] = x[e]; dycf[r][e] = y[e]; mu[r][e] = 0; mv[r][e] = 0; }
            if (masked) {                                          // a count plane has no halo: clamped onto the last interior row
                const long long n0 = (long long)a.Nx * (j0 + min(r, nr - 1)) + e0;
                const Counts<W> nu = *reinterpret_cast<const Counts<W>*>(p.nfc + n0);
                const Counts<W> nv = *reinterpret_cast<const Counts<W>*>(p.ncf + n0);
#pragma unroll
                for (int e = 0; e < W; ++e) {                      // masked levels (0-based k < m)
                    mu[r][e] = min(max(nu[e], 0), a.Nz);
                    mv[r][e] = min(max(nv[e], 0), a.Nz);
                }
            }
        }
        if constexpr (COR != 0) {
            const T* px = static_cast<const T*>(p.dxcf) + m0;      // rows 0 .. JT, columns -1 .. W - 1
            const T* ff = static_cast<const T*>(p.f) + m0;         // rows 0 .. JT, columns 0 .. W (row JT: 0 .. W - 1)
#pragma unroll
            for (int r = 0; r <= JT; ++r) {
                const cvec_t x = chunk(px + ro[r + 1]), c = chunk(ff + ro[r + 1]);
                dxcf[r][0] = px[ro[r + 1] - 1];
#pragma unroll
                for (int e = 0; e < W; ++e) { dxcf[r][e + 1] = x[e]; f[r][e] = c[e]; }
                if (r < JT) f[r][W] = ff[ro[r + 1] + W];
            }
            const T* qy = static_cast<const T*>(p.dyfc) + m0;      // rows -1 .. JT - 1, columns 0 .. W
#pragma unroll
            for (int r = -1; r < JT; ++r) {
                const cvec_t y = chunk(qy + ro[r + 1]);
                dyfc[r + 1][W] = qy[ro[r + 1] + W];
#pragma unroll
                for (int e = 0; e < W; ++e) dyfc[r + 1][e] = y[e];
            }
        }
    }

    const long long f0 = a.off3 + (long long)a.sx * j0 + e0;
    const T* u = static_cast<const T*>(p.u) + f0;
    const T* v = static_cast<const T*>(p.v) + f0;
    const T* b = static_cast<const T*>(p.b) + f0;
    const T* dz = static_cast<const T*>(p.dz);
    T* Gu = static_cast<T*>(p.Gu) + f0;
    T* Gv = static_cast<T*>(p.Gv) + f0;
    T* po = static_cast<T*>(p.p) + f0;
    const T mval = (T)a.value;

    // b of one level at the cells whose PH the item carries: rows -1 .. JT - 1, columns -1 .. W - 1, without (-1, -1); the row south only
    // where a py needs it, the column west only where it is this lane's own
    auto load_b = [&](T (&x)[JT + 1][W + 1], const T* bk) {
#pragma unroll
        for (int r = -1; r < JT; ++r) {
            if (r < 0 && !hasG) continue;
            const cvec_t c = chunk(bk + ro[r + 1]);
#pragma unroll
            for (int e = 0; e < W; ++e) x[r + 1][e + 1] = c[e];
            if (r >= 0 && hasG && own_west) x[r + 1][0] = bk[ro[r + 1] - 1];
        }
    };

    struct Level {
        T b[JT + 1][W + 1];                                        // rows -1 .. JT - 1, columns -1 .. W - 1
        T v[JT + 1][W + 1];                                        // rows 0 .. JT, columns -1 .. W - 1
        T u[JT + 1][W + 1];                                        // rows -1 .. JT - 1, columns 0 .. W
        T gu[JT][W], gv[JT][W];                                    // ADD: what Gu, Gv hold at the nodes
        T d;                                                       // dz_f of the level's top face
    };
    auto load = [&](Level& L, int k) {
        if constexpr (PRES) {
            L.d = dz[k + 1];
            load_b(L.b, b + a.plane * k);
        }
        if constexpr (COR != 0) {
            const T* uk = u + a.plane * k;
            const T* vk = v + a.plane * k;
#pragma unroll
            for (int r = 0; r <= JT; ++r) {
                const cvec_t y = chunk(vk + ro[r + 1]), x = chunk(uk + ro[r]);
                L.v[r][0] = vk[ro[r + 1] - 1];
                L.u[r][W] = uk[ro[r] + W];
#pragma unroll
                for (int e = 0; e < W; ++e) { L.v[r][e + 1] = y[e]; L.u[r][e] = x[e]; }
            }
        }
        if (add) {
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                const cvec_t x = chunk(Gu + a.plane * k + ro[r + 1]), y = chunk(Gv + a.plane * k + ro[r + 1]);
#pragma unroll
                for (int e = 0; e < W; ++e) { L.gu[r][e] = x[e]; L.gv[r][e] = y[e]; }
            }
        }
    };

    // carried down the column: PH of the level above and b there, at the cells of load_b
    T PH[JT + 1][W + 1] = {}, bup[JT + 1][W + 1];
    if constexpr (PRES) load_b(bup, b + a.plane * a.Nz);           // the top halo plane

    Level ring[LA];
#pragma unroll
    for (int s = 0; s < LA; ++s) load(ring[s], max(a.Nz - 1 - s, 0));
    for (int q0 = 0; q0 < a.Nz; q0 += LA) {
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int q = q0 + s;
            if (q >= a.Nz) break;
            const int k = a.Nz - 1 - q;                            // the level, 0-based: top-down
            Level L = ring[s];
            if (q + LA < a.Nz) load(ring[s], k - LA);              // the loads of level k - LA go out before level k's arithmetic
            if constexpr (PRES) {
#pragma unroll
                for (int r = 0; r <= JT; ++r)
#pragma unroll
                    for (int c = 0; c <= W; ++c) {
                        if ((r == 0 && c == 0) || (r == 0 && !hasG) || (c == 0 && !(hasG && own_west))) continue;
                        const T x = (half * (L.b[r][c] + bup[r][c])) * L.d;
                        PH[r][c] = q == 0 ? -x : PH[r][c] - x;
                        bup[r][c] = L.b[r][c];
                    }
                if constexpr (SHARE) {
#pragma unroll
                    for (int r = 0; r < JT; ++r) {
                        const T west = __shfl_up(PH[r + 1][W], 1);
                        if (!own_west) PH[r + 1][0] = west;
                    }
                }
            }
            // P: rows 0 .. JT, columns -1 .. W - 1.  Q: rows -1 .. JT - 1, columns 0 .. W
            T P[JT + 1][W + 1], Q[JT + 1][W + 1];
            if constexpr (COR != 0) {
#pragma unroll
                for (int r = 0; r <= JT; ++r)
#pragma unroll
                    for (int e = 0; e <= W; ++e) { P[r][e] = dxcf[r][e] * L.v[r][e]; Q[r][e] = dyfc[r][e] * L.u[r][e]; }
            }
#pragma unroll
            for (int r = 0; r < JT; ++r) {
                if (r >= nr) break;
                const long long at = a.plane * k + (long long)a.sx * r;
                if constexpr (PRES) {
                    if (a.hasP) {
                        cvec_t ph;
#pragma unroll
                        for (int e = 0; e < W; ++e) ph[e] = PH[r + 1][e + 1];
                        store_chunk<NT>(reinterpret_cast<cvec_t*>(po + at), ph);
                    }
                }
                if (!hasG) continue;
                cvec_t gu, gv;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    T cu = T(0), cv = T(0), px = T(0), py = T(0);
                    if constexpr (COR == 1) {
                        const T fu = half * (f[r][e] + f[r + 1][e]);
                        const T vh = half * (half * (P[r][e] + P[r + 1][e]) + half * (P[r][e + 1] + P[r + 1][e + 1]));
                        cu = (fu * vh) / dxfc[r][e];
                        const T fv = half * (f[r][e] + f[r][e + 1]);
                        const T uh = half * (half * (Q[r][e] + Q[r][e + 1]) + half * (Q[r + 1][e] + Q[r + 1][e + 1]));
                        cv = (fv * uh) / dycf[r][e];
                    }
                    if constexpr (COR == 2) {
                        const T vx0 = half * (P[r][e] + P[r][e + 1]), vx1 = half * (P[r + 1][e] + P[r + 1][e + 1]);
                        cu = (half * (f[r][e] * vx0 + f[r + 1][e] * vx1)) / dxfc[r][e];
                        const T uy0 = half * (Q[r][e] + Q[r + 1][e]), uy1 = half * (Q[r][e + 1] + Q[r + 1][e + 1]);
                        cv = (half * (f[r][e] * uy0 + f[r][e + 1] * uy1)) / dycf[r][e];
                    }
                    if constexpr (PRES) {
                        px = (PH[r + 1][e + 1] - PH[r + 1][e]) / dxfc[r][e];
                        py = (PH[r + 1][e + 1] - PH[r][e + 1]) / dycf[r][e];
                    }
                    T x, y;
                    if constexpr (COR != 0 && PRES) {
                        x = add ? (L.gu[r][e] + cu) - px : cu - px;
                        y = add ? (L.gv[r][e] - cv) - py : (-cv) - py;
                    } else if constexpr (COR != 0) {
                        x = add ? L.gu[r][e] + cu : cu;
                        y = add ? L.gv[r][e] - cv : -cv;
                    } else {
                        x = add ? L.gu[r][e] - px : -px;
                        y = add ? L.gv[r][e] - py : -py;
                    }
                    gu[e] = k < mu[r][e] ? mval : x;
                    gv[e] = k < mv[r][e] ? mval : y;
                }
                store_chunk<NT>(reinterpret_cast<cvec_t*>(Gu + at), gu);
                store_chunk<NT>(reinterpret_cast<cvec_t*>(Gv + at), gv);
            }
        }
    }
}

}  // namespace

extern "C" {

// this library links its own copy of the error channel (tpg_api.hip): the message of the last failure of a call into THIS library
const char* tpg_hydrostatic_last_error(void) { return tpg_last_error(); }

int tpg_hydrostatic_tendencies(const void* u, const void* v, const void* b, void* Gu, void* Gv, void* p_out, const void* f_ff, const void* dx_fc,
                               const void* dy_fc, const void* dx_cf, const void* dy_cf, const void* dz_f, const int32_t* n_fc, const int32_t* n_cf,
                               double mask_value, int coriolis_scheme, int mode, int Nx, int Ny, int Nz, int Hx, int Hy, int Hz, int ft, void* stream)
{
    if (int rc = tpg::check_geom(Nx, Ny, Nz, Hx, Hy, Hz, ft)) return rc;
    if (coriolis_scheme != TPG_CORIOLIS_ENSTROPHY_CONSERVING && coriolis_scheme != TPG_CORIOLIS_ENERGY_CONSERVING) {
        tpg::set_error("Coriolis scheme %d is not built (TPG_CORIOLIS_ENSTROPHY_CONSERVING = 0 and TPG_CORIOLIS_ENERGY_CONSERVING = 1 are; "
                       "ActiveCellEnstrophyConserving is not)", coriolis_scheme);
        return TPG_ERR_UNSUPPORTED;
    }
    if (mode != TPG_TENDENCY_ADD && mode != TPG_TENDENCY_WRITE) {
        tpg::set_error("tendency mode %d is not built (TPG_TENDENCY_ADD = 0 and TPG_TENDENCY_WRITE = 1 are)", mode);
        return TPG_ERR_UNSUPPORTED;
    }
    if (!f_ff && !b) { tpg::set_error("neither f_ff nor b: no term to compute"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!Gu != !Gv) { tpg::set_error("Gu and Gv are given together or not at all (%s is null)", Gu ? "Gv" : "Gu"); return TPG_ERR_INVALID_ARGUMENT; }
    const bool hasG = Gu != nullptr;
    if (!hasG && (!b || !p_out)) { tpg::set_error("without Gu and Gv the call is the pressure alone: b and p_out needed"); return TPG_ERR_INVALID_ARGUMENT; }
    if (p_out && !b) { tpg::set_error("p_out without b"); return TPG_ERR_INVALID_ARGUMENT; }
    if (hasG && (!dx_fc || !dy_cf)) { tpg::set_error("null dx_fc or dy_cf"); return TPG_ERR_INVALID_ARGUMENT; }
    const bool cor = hasG && f_ff;
    if (cor && (!u || !v || !dx_cf || !dy_fc)) { tpg::set_error("f_ff without u, v, dx_cf or dy_fc"); return TPG_ERR_INVALID_ARGUMENT; }
    if (b && !dz_f) { tpg::set_error("b without dz_f"); return TPG_ERR_INVALID_ARGUMENT; }
    if (!n_fc != !n_cf) { tpg::set_error("the count planes n_fc and n_cf are given together or not at all (%s is null)", n_fc ? "n_cf" : "n_fc"); return TPG_ERR_INVALID_ARGUMENT; }
    const size_t esz = elem_size(ft);
    if (misaligned(esz, u, v, b)) { tpg::set_error("u, v or b pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(esz, Gu, Gv, p_out)) { tpg::set_error("Gu, Gv or p_out pointer not aligned to its element type"); return TPG_ERR_INVALID_ARGUMENT; }
    if (misaligned(esz, f_ff, dx_fc, dy_fc, dx_cf, dy_cf, dz_f)) {
        tpg::set_error("f_ff, dx_fc, dy_fc, dx_cf, dy_cf or dz_f pointer not aligned to its element type");
        return TPG_ERR_INVALID_ARGUMENT;
    }
    if ((uintptr_t)n_fc % 4 || (uintptr_t)n_cf % 4) { tpg::set_error("count plane pointer not aligned to int32"); return TPG_ERR_INVALID_ARGUMENT; }
    const Geom g = tpg::make_geom(Nx, Ny, Nz, Hx, Hy, Hz);
    const unsigned long long bytes = (unsigned long long)g.plane * (g.Nz + 2 * g.Hz) * esz;
    const Span spans[6] = { { Gu, bytes, "Gu", true }, { Gv, bytes, "Gv", true }, { p_out, bytes, "p_out", true },
                            { u, bytes, "u", false }, { v, bytes, "v", false }, { b, bytes, "b", false } };
    if (int rc = check_overlaps(spans, 6, "every item reads cells while its neighbours write")) return rc;
    if (g.Hx < 1 || g.Hy < 1 || g.Hz < 1) {
        tpg::set_error("the rule reads u, v, b[i-1..i+1, j-1..j+1] and b[k..Nz+1]: Hx >= 1, Hy >= 1 and Hz >= 1 needed (halo (%d,%d,%d))", g.Hx, g.Hy, g.Hz);
        return TPG_ERR_UNSUPPORTED;
    }
    const int JT = ft == TPG_F64 ? ROWS<double> : ROWS<float>;
    const long long tiles = (g.Ny + JT - 1) / JT;
    if (tiles * (g.Nx / 2) >= (1ll << 31) - 256) { tpg::set_error("hydrostatic tendencies: too many work items for 32-bit indexing"); return TPG_ERR_UNSUPPORTED; }

    const bool masked = hasG && n_fc;
    const HydrostaticPtrs p{ cor ? u : nullptr, cor ? v : nullptr, b, Gu, Gv, p_out, cor ? f_ff : nullptr, dx_fc, cor ? dy_fc : nullptr,
                             cor ? dx_cf : nullptr, dy_cf, dz_f, masked ? n_fc : nullptr, masked ? n_cf : nullptr };
    // every array whose chunks the kernel touches, for chunk_plan (a null pointer is on every grid)
    void* all[11];
    int na = 0;
    for (const void* x : { p.u, p.v, p.b, (const void*)p.Gu, (const void*)p.Gv, (const void*)p.p, p.f, hasG ? p.dxfc : nullptr, p.dyfc, p.dxcf,
                           hasG ? p.dycf : nullptr })
        all[na++] = const_cast<void*>(x);
    hipStream_t st = tpg::as_stream(stream);
    return dispatch_ft(ft, [&](auto ty) {
        typedef decltype(ty) T;
        const ChunkPlan cp = chunk_plan<T>(g, all, na);
        const int cpr = g.Nx / cp.W;
        const HydrostaticArgs a{ g.Nx, g.Ny, g.Nz, g.sx, cpr, (int)(tiles * cpr), g.plane, interior2(g), interior3(g),
                                 masked ? (double)(T)mask_value : 0.0, hasG && mode == TPG_TENDENCY_ADD, masked, hasG, p_out != nullptr };
        const unsigned blocks = (unsigned)((a.items + 255) / 256);
        dispatch_chunk<T>(cp.W, cp.gen, [&](auto cw, auto gen) {
            auto go = [&](auto c, auto pres) {
                hipLaunchKernelGGL((k_hydrostatic_tendencies<T, decltype(cw)::value, decltype(gen)::value, decltype(c)::value, decltype(pres)::value,
                                                             ROWS<T>, LOOKAHEAD>), dim3(blocks), dim3(256), 0, st, p, a);
            };
            typedef std::integral_constant<int, 0> none_t;
            typedef std::integral_constant<int, 1> enstrophy_t;
            typedef std::integral_constant<int, 2> energy_t;
            if (!cor)                                                     go(none_t{}, std::true_type{});
            else if (coriolis_scheme == TPG_CORIOLIS_ENSTROPHY_CONSERVING) { if (b) go(enstrophy_t{}, std::true_type{}); else go(enstrophy_t{}, std::false_type{}); }
            else                                                          { if (b) go(energy_t{}, std::true_type{}); else go(energy_t{}, std::false_type{}); }
        });
        return tpg::launch_status("k_hydrostatic_tendencies");
    });
}

}  // extern "C"
