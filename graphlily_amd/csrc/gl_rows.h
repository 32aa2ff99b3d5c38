// The plain CSR row copy that a GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base), as the
// graph kernels that walk it see it -- gl_bfs_parents, gl_cc, gl_tc, gl_kcore, gl_color, gl_truss, gl_msf (which also takes a
// value per entry of the copy from its caller), gl_bc: what a caller may require of it, the
// verdicts about it that the plan caches, and the few helpers every such kernel wants.  gl_rows.hip holds the check kernels.
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

// the grid of a streaming pass, a thread per vertex
inline unsigned rows_stream_grid(uint32_t n) { return std::max(1u, std::min<unsigned>(cdiv(n, 256u), (unsigned)ctx().num_cus * 8u)); }
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

}  // namespace gl

#endif  // GL_ROWS_H_
