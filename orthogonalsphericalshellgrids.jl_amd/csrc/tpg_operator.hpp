// tpg_operator.hpp -- what the operator translation units share (tpg_operators.hip, tpg_continuity.hip, tpg_barotropic.hip,
// tpg_free_surface.hip, tpg_timestep.hip and, through tpg_tracer_tendency.hpp, tpg_advection.hip, tpg_weno.hip and tpg_weno_xyz.hip, through
// tpg_momentum_tendency.hpp, tpg_momentum.hip and tpg_weno_momentum.hip; each is a library of its own): the chunk and count access types and the store of their kernels, and the arithmetic, the Span record and the overlap
// check their entry points check arguments with.  An entry point keeps its own sequence of checks, statuses and messages; a new operator
// starts here.
#pragma once
#include "tpg_launch.hpp"

namespace {

// the chunk of W elements the kernels load and store: 16-B aligned, or (GEN) element-aligned -- chunk_plan's plain / GEN split
template <typename T, int W, bool GEN>
using Chunk = typename std::conditional<GEN, typename Vec<T, W>::loose_t, typename Vec<T, W>::aligned_t>::type;

// the W int32 column counts under a chunk: a count plane is Nx x Ny without halos, so element-aligned always
template <int W> struct CountsOf { typedef int type __attribute__((ext_vector_type(W), aligned(4))); };
template <int W> using Counts = typename CountsOf<W>::type;

// the store of an output chunk: streaming (non-temporal) or ordinary, by each file's compile-time switch (TPG_VORT_NT, TPG_CONT_NT, TPG_BARO_NT)
template <bool NT, typename V>
__device__ __forceinline__ void store_chunk(V* p, V v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// bytes of an element of type ft (validated by tpg::check_geom)
size_t elem_size(int ft) { return ft == TPG_F64 ? 8 : 4; }

// any of the pointers off the esz-byte grid (a null pointer is on it)
template <typename... P>
bool misaligned(size_t esz, P... p) { return ((uintptr_t)0 | ... | (uintptr_t)p) % esz != 0; }

// the arrays [p, p + pbytes) and [q, q + qbytes) share a byte
bool arrays_overlap(const void* p, unsigned long long pbytes, const void* q, unsigned long long qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b ? b - a < pbytes : a - b < qbytes;
}

// an array of a call: where it is, how long, what the messages call it, whether the call writes it
struct Span { const void* p; unsigned long long bytes; char name[24]; bool written; };

// any written array against every other array of the call.  A call whose messages or order differ keeps its own loop (the tracer tendencies,
// tpg_tracer_tendency.hpp; the momentum tendencies, tpg_momentum_tendency.hpp)
int check_overlaps(const Span* s, int n, const char* why)
{
    for (int o = 0; o < n; ++o) {
        if (!s[o].p || !s[o].written) continue;
        for (int q = 0; q < n; ++q)
            if (q != o && s[q].p && arrays_overlap(s[o].p, s[o].bytes, s[q].p, s[q].bytes)) {
                tpg::set_error("%s overlaps %s (%s)", s[o].name, s[q].name, why);
                return TPG_ERR_INVALID_ARGUMENT;
            }
    }
    return TPG_OK;
}

// the first interior cell of a padded plane (sx * Hy + Hx) and of a 3-D parent (plane * Hz + that)
long long interior2(const Geom& g) { return (long long)g.sx * g.Hy + g.Hx; }
long long interior3(const Geom& g) { return g.plane * g.Hz + interior2(g); }

}  // namespace
