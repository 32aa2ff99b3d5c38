// The plain CSR row copy that a GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base), as the
// graph kernels that walk it see it -- gl_bfs_parents, gl_cc, gl_tc, gl_kcore, gl_color, gl_truss, gl_bc, gl_scc, gl_bicc, gl_topo, gl_msbfs, gl_sim, gl_lpa, and gl_msf,
// gl_match and gl_louvain (which also take a value per entry of the copy from their caller): what a caller may require of it,
// the verdicts about it that the plan caches, the few helpers every such kernel wants, and the walk over a row -- a thread per
// row, then the wavefront -- that ten of them run and gl_bc copies (rows_walk_*, at the end; gl_tc, gl_truss and gl_sim intersect rows
// instead).  gl_rows.hip holds the check kernels.  A new caller adds itself to tests/test_gpu_rows.py (the contract) and
// tests/test_gpu_walk.py (the walk).
// gl_rounds.h, on top of this, holds what the kernels that run in rounds over a queue share: the atomics of their memory rule,
// the queue append, the peel record and the gated host loop.
#ifndef GL_ROWS_H_
#define GL_ROWS_H_

#include "gl_spmv_plan.h"

namespace gl {

// row r of [row_begin, row_begin + rows) holds the entries row_idx[row_ptr[r - row_begin] - nz_base .. row_ptr[r - row_begin + 1]
// - nz_base): columns below num_cols, or 0xffffffff for a zero-valued entry
struct RowsView {
    const uint32_t *row_ptr, *row_idx;
    uint32_t nz_base, row_begin, rows, num_cols;
};
inline RowsView rows_view(gl_spmv_plan p) {
    return {p->d_csr_indptr, p->d_csr_indices, p->csr_nz_base, p->row_begin, p->row_end - p->row_begin, p->num_cols};
}

// What a caller needs of the plan's row copy.  The last three are nested: each asks for the one before it.
enum : unsigned {
    kRowsIndexable = 1u,               // a row copy whose rows are columns too: row_end <= num_cols
    kRowsSquare = 2u,                  // square, the whole matrix, entries that fit 32-bit offsets; a matrix WITHOUT entries
                                       // keeps no row copy and is accepted here (and needs nothing further)
    kRowsSets = 4u | kRowsSquare,      // ... whose rows are strictly ascending sets of columns below num_cols
    kRowsSymmetric = 8u | kRowsSets,   // ... and hold (u, v) for every (v, u)
};
// The refusals (GL_ERR_UNSUPPORTED), in this order; the verdicts asked for are established on first use -- one kernel and one
// synchronisation each -- and cached in the plan.  `which` names the plan in the messages ("the plan", "plan_in"), `hint` the
// io.* helper that prepares a matrix the caller accepts.
int rows_require(gl_spmv_plan p, unsigned need, const char *who, const char *which, const char *hint = nullptr);
// -> p->rows_sorted, on first use: do the valid columns of every row ascend?  (a plan that passed kRowsIndexable)
int rows_check_sorted(gl_spmv_plan p);
// is (u, v) stored in `partner` for every entry (v, u) of p?  Both plans passed kRowsSets and have entries and as many rows.
// partner == p asks whether the pattern is symmetric (diagonal entries are then not looked up): kRowsSymmetric's verdict.
int rows_check_transpose(gl_spmv_plan p, gl_spmv_plan partner, bool *ok);
// The refusals of the calls that take a pattern as TWO plans, plan_in (row v: the vertices v is pulled from) and plan_out (the
// transposed pattern; plan_out == plan_in declares the pattern symmetric) -- gl_bc_accumulate, gl_scc, gl_topo -- in this order:
// rows_require(plan_in, kRowsSymmetric if the two are one plan, else kRowsSets), rows_require(plan_out, kRowsSets), as many
// vertices, and plan_out IS the transpose: as many entries and rows_check_transpose, whose verdict plan_in caches for the last
// partner (by handle and uid).  All GL_ERR_UNSUPPORTED.
int rows_require_pair(gl_spmv_plan pin, gl_spmv_plan pout, const char *who, const char *hint);

// the grid of a streaming pass, a thread per vertex
inline unsigned rows_stream_grid(uint32_t n) { return std::max(1u, std::min<unsigned>(cdiv(n, 256u), (unsigned)ctx().num_cus * 8u)); }
// the launch of a walk (below) over `items` rows, 64 per wavefront, from its caller's two A/B knobs: `cut` = entries a thread reads
// before the wavefront takes the row over (0 .. cut_cap, in steps of four), `per_cu` = workgroups per compute unit (1 .. 1024)
struct RowsWalkShape {
    uint32_t cut_steps;
    unsigned grid;
};
inline RowsWalkShape rows_walk_shape(uint32_t items, long cut, long cut_cap, long per_cu) {
    const unsigned most = (unsigned)ctx().num_cus * (unsigned)std::max<long>(1, std::min<long>(per_cu, 1024));
    return {(uint32_t)std::max<long>(0, std::min<long>(cut, cut_cap)) / 4u, std::max(1u, std::min<unsigned>(cdiv(items, 256u), most))};
}
// d_out[v] = v for v < n, n >= 1: one launch (the answer of the calls that find a graph without entries)
int rows_iota(uint32_t *d_out, uint32_t n);

// scratch that its first user allocates and its owner (a plan, the context) frees
template <typename T>
int plan_scratch(T *&slot, size_t bytes, const char *who, const char *what) {
    if (slot) return GL_OK;
    const hipError_t e = hipMalloc((void **)&slot, bytes);
    if (e != hipSuccess) return set_error(GL_ERR_HIP, "%s: hipMalloc(%zu bytes of %s): %s", who, bytes, what, hipGetErrorString(e));
    return GL_OK;
}

// position of the first entry >= w in the ascending s[0 .. n), n >= 1; the result is < n
template <typename P>
__device__ __forceinline__ uint32_t rows_lower_bound(P s, uint32_t n, uint32_t w) {
    uint32_t lo = 0;
    while (n > 1u) {
        const uint32_t half = n >> 1;
        lo += s[lo + half - 1u] < w ? half : 0u;
        n -= half;
    }
    return lo;
}

// THE WALK over the entries [beg, end) of one row per lane, 64 rows per wavefront (gl_bfs_parents, gl_cc, gl_kcore, gl_msf, gl_match,
// gl_color, gl_scc, gl_bicc, gl_topo and gl_msbfs run all of it -- match_collect_kernel with a copy of the thread steps in which every lane takes every step --,
// gl_lpa and gl_louvain the takeover and the wavefront's steps behind a thread path of their own; DESIGN.md 4.13.  bc_sweep_kernel of
// gl_bc keeps a copy of its own, in the same forms: through these templates its accumulate figure on one stand-in was 1 - 2 % above
// the parent's worse run in two visits, EXPERIMENTS.md Round 21):
//   rows_walk_thread    a thread per row, four entries per step, for at most cut_steps steps while any lane of the wavefront has
//                       entries left: body(c, beg) gets the columns of the entries beg .. beg + 3 and returns true when the row
//                       needs no further entry (the row is then finished: beg = end); beg moves on behind what was read
//   rows_walk_takeover  every row still unfinished (beg < end) is taken over by the whole wavefront, one row after the other in
//                       lane order: per_row(src, b, e) gets the lane that owns the row and that lane's beg and end; whatever
//                       else of that lane the caller needs it shuffles from src itself
//   rows_walk_wave      the wavefront reads [b, e) 256 entries per step, lane l the entries base + l, base + 64 + l, base + 128 + l
//                       and base + 192 + l (coalesced index loads): body(c, base) returns true -- the same in every lane -- to stop
// PADDING: a position at or behind the row's end reads no memory and has the column 0xffffffff, which is also the column of a
// zero-valued entry and is below no num_cols: a body's test `c[u] < n` drops both.
// NO WRAP, whatever the offsets (a row may end at entry 2^32 - 1): the thread tests `end - beg > u` (never beg + u < end) and
// advances by min(4, end - beg), so no offset is formed behind end; the wavefront's base and positions are 64-bit, below 2^32 + 256.
// Everything a body loads beside the columns (levels, weights) it loads first thing, so that those loads and the index loads of
// the step are in flight together; a body that never stops early returns a constant false, which costs nothing.
template <typename Body>
__device__ __forceinline__ void rows_walk_thread(const uint32_t *__restrict__ row_idx, uint32_t &beg, uint32_t end, uint32_t cut_steps,
                                                 Body &&body) {
    for (uint32_t step = 0; step < cut_steps && __any(beg < end); step++) {
        if (beg < end) {
            uint32_t c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) c[u] = end - beg > (uint32_t)u ? row_idx[beg + u] : 0xffffffffu;
            beg = body(c, beg) ? end : beg + min(4u, end - beg);
        }
    }
}
template <typename PerRow>
__device__ __forceinline__ void rows_walk_takeover(uint32_t beg, uint32_t end, PerRow &&per_row) {
    for (uint64_t pending = __ballot(beg < end); pending; pending &= pending - 1ull) {
        const int src = __ffsll((unsigned long long)pending) - 1;
        per_row(src, (uint32_t)__shfl(beg, src), (uint32_t)__shfl(end, src));
    }
}
template <typename Body>
__device__ __forceinline__ void rows_walk_wave(const uint32_t *__restrict__ row_idx, uint32_t b, uint32_t e, uint32_t lane, Body &&body) {
    for (uint64_t base = b; base < e; base += 256u) {
        uint32_t c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t j = base + 64u * u + lane;
            c[u] = j < e ? row_idx[j] : 0xffffffffu;
        }
        if (body(c, base)) break;
    }
}

}  // namespace gl

#endif  // GL_ROWS_H_
