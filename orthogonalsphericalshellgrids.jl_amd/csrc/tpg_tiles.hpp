// tpg_tiles.hpp -- the integer arithmetic of k_cells_tile's prologue (csrc/tpg_grid.hip): block id -> tile -> (tile row, tile column), and
// the stored column of a strip lane.  Every wave of a launch runs it before its first Float64 instruction, so it holds no division: what
// depends on the launch alone comes from the host as a kernel argument.  Plain integer C++ in a header of its own, so that
// tests/test_cells_prologue.py can compile it for the host and hold it against `/` and `%` exhaustively.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPG_HD __host__ __device__ __forceinline__
#else
#define TPG_HD inline
#endif

namespace tpgt {

// ---- tile order ------------------------------------------------------------------------------------------------------------------
// XCD-grouped order: a permutation inside every whole group of 64 block ids that gives the ids with one value of id mod 8 -- one XCD's
// blocks -- 8 consecutive tiles; the ids of a last, partial group keep their own tile.  grouped = false: the identity (TPG_CELLS_ORDER 0)
TPG_HD int tile_of_block(int b, int tiles, bool grouped)
{
    const int base = b & ~63;
    if (grouped && base + 64 <= tiles) return base + (b & 7) * 8 + ((b >> 3) & 7);
    return b;
}

// ---- t / d and t % d without a division --------------------------------------------------------------------------------------------
// The host passes rcp = floor((2^32 - 1) / d), d >= 1.  With delta = 2^32 / d - rcp, 0 < delta <= 1 (d = 1 and the powers of two give 1),
// t rcp / 2^32 = t / d - t delta / 2^32 lies in (t / d - 1, t / d] for every t < 2^32: the high word of the product is the quotient or
// one less, never more, and ONE conditional step mends it.  Any t and d of 32 bits, so in particular every tile number below
// tiles = tiles_x tiles_y < 2^31.  On wave-uniform operands: s_mul_hi_u32, s_mul_i32, s_sub, s_cmp and two selects.
inline unsigned rcp_of(unsigned d) { return 0xFFFFFFFFu / d; }        // host side

struct DivMod { unsigned q, r; };
TPG_HD DivMod divmod_rcp(unsigned t, unsigned d, unsigned rcp)
{
    const unsigned q = (unsigned)(((unsigned long long)t * rcp) >> 32);
    const unsigned r = t - q * d;                     // in [0, 2 d)
    // the step as sign arithmetic, d < 2^31: below = -1 where r < d, else 0.  (Written as a compare and two selects, the compiler takes the
    // carry into the quotient through a vector register and back.)
    const int over = (int)(r - d), below = over >> 31;
    return DivMod{ q + 1u + (unsigned)below, (unsigned)over + (d & (unsigned)below) };
}

// tile t -> tile row ty (tile rows are counted NORTH to SOUTH in t) and tile column tx
struct TileXY { int tx, ty; };
TPG_HD TileXY tile_xy(int t, int tiles_x, int tiles_y, unsigned tiles_x_rcp)
{
    const DivMod dm = divmod_rcp((unsigned)t, (unsigned)tiles_x, tiles_x_rcp);
    return TileXY{ (int)dm.r, tiles_y - 1 - (int)dm.q };
}

// ---- stored column of a strip lane, wrapped into 1..Nx ------------------------------------------------------------------------------
// The ascending strip of tile tx holds v = shift + 30 tx + hl, its image v = shift - 30 tx - 30 + hl, with shift = Nx / 4, 0 <= hl <= 31 and
// tx < ceil((Nx / 2) / 30), so -Nx / 4 - 59 <= v <= 3 Nx / 4 + 61: from Nx = 80 on, one period either way brings every v into 1..Nx.
// Narrower grids can be more than one period away and take the generic modulo.  The test of the width is wave-uniform (a scalar
// compare and branch), so the ordinary grid pays nothing else for the generic path.
constexpr int kWrapOnePeriodNx = 128;      // >= 80 with room to spare
TPG_HD int wrap_col(int v, int Nx)
{
    if (v < 1) v += Nx;
    if (v > Nx) v -= Nx;
    if (Nx < kWrapOnePeriodNx) {
        if (v < 1 || v > Nx) { v = (v - 1) % Nx; v = (v < 0 ? v + Nx : v) + 1; }
    }
    return v;
}

}  // namespace tpgt
