/*
 * graphlily_hip_spgemm.h -- the sparse matrix product extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry points of gl_spgemm.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_SPGEMM_H_
#define GRAPHLILY_HIP_SPGEMM_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the mask admits (i, j) when (i, j) is NOT stored in `mask` */
#define GL_SPGEMM_MASK_COMPLEMENT 1u

/* SpGEMM, C = A (+).(x) B with a sparse result and an optional structural mask, over the plain CSR copies that GL_PLAN_BOOLEAN
 * plans keep (gl_spgemm.hip).  a, b and mask are square, whole-matrix plans over the same n vertices whose rows
 * are strictly ascending sets of columns (built from all-ones values, as for gl_msf: a zero VALUE is a legitimate value here, and
 * the values travel apart from the plans).  a == b, mask == a and mask == b are legal.
 *
 * THE PATTERN OF C IS STRUCTURAL: row i of C holds column j exactly when some k has (i, k) in a and (k, j) in b and the mask
 * admits (i, j) -- (i, j) stored in `mask`; with GL_SPGEMM_MASK_COMPLEMENT: not stored; without a mask: always.  Nothing is
 * dropped by value: an entry that comes out as 0.0 or +inf stays an entry.  The columns of every row of C are strictly
 * ascending and d_c_indptr[0] = 0.  The caller cannot size C before the symbolic call has run:
 *
 *   gl_spgemm_symbolic  writes the n + 1 words of d_c_indptr and SYNCHRONISES.  h_stats (4 HOST words, required) =
 *                       {nnz(C), products, rows that took the workgroup path, rows that took the slab path}; products = the sum
 *                       over the entries (i, k) of a of |b(k)|.  nnz(C) >= 2^32 is GL_ERR_UNSUPPORTED.
 *   gl_spgemm_numeric   takes the d_c_indptr that a symbolic call with the same plans, mask and flags wrote and writes the
 *                       nnz(C) words of d_c_indices and of d_c_val.  d_a_val[j] / d_b_val[j] is the f32 value of entry j of the
 *                       plan's row copy, in the caller's order.  `semiring` is a gl_op.  IT ONLY ENQUEUES, unless h_stats
 *                       (4 HOST words, may be NULL: the same four figures, the paths now chosen by |C(i)|) is given.
 *                       Under GL_OP_ANDOR no value is read: d_a_val, d_b_val and d_c_val may be NULL, and a d_c_val that
 *                       is given receives 1.0 per entry.
 * Nothing behind word n + 1 of d_c_indptr and nothing behind word nnz(C) of d_c_indices or d_c_val is written.  If a or b
 * has no entries (or a mask without entries must admit), C has none: d_c_indptr is written as zeros by one launch, and no row
 * takes a path; `products` does not depend on the mask and is reported all the same.
 *
 * ARITHMETIC.  (min,+) forms a + b in f32 and takes the minimum through the monotone map of f32 to uint32 that gl_msf uses
 * (integer atomics): the result is bit-exact whatever the schedule.  (+,x) forms every product in f64 -- the product of two f32
 * values is exact in f64 --, adds in f64 and rounds to f32 ONCE, at emission; no f32 atomic is used anywhere.  So
 * |c - exact| <= 2^-24 |exact| + p 2^-52 sum|a b| + 2^-149 for an entry of p products.  The library reads the values as they
 * are; the drivers refuse NaN for every semiring and +-inf for (+,x).
 *
 * HOW: row-wise (Gustavson), one agent per row of C, the columns of the rows b(k), k in a(i), inserted into a table of
 * (column, accumulator) slots -- claimed by compare-and-swap on the empty key 0xffffffff, linear probing -- with the mask
 * applied at insertion.  Three paths, chosen per row by a count (symbolic: the row's products, an upper bound; numeric: |C(i)|
 * itself): a wavefront with a table of GRAPHLILY_DEBUG spgemm_wave_slots (512) slots in LDS while the count fits; a workgroup
 * with spgemm_lds_slots (8192) slots in dynamic LDS; a dense accumulator over the n columns (a bitmap and a 64-bit word per
 * column) in one of a fixed number of global slabs.  spgemm_wave=0 / spgemm_lds=0 close the first / the first two paths.  The
 * hash paths compact the occupied slots and sort them in LDS (by counting up to 64 entries, a bitonic network above); the slab
 * emits from its bitmap, which is in column order.  The plan `a` caches the bounds, the symbolic bins, the knobs and the slabs
 * for its last partner `b` (by handle and uid); its first call with a partner waits once.
 *
 * GL_ERR_INVALID_ARG: a NULL a, b, d_c_indptr, or symbolic h_stats; flags beyond GL_SPGEMM_MASK_COMPLEMENT, or that flag
 * without a mask; a semiring that is no gl_op; a NULL d_c_indices; a NULL d_a_val, d_b_val or d_c_val under (+,x) or (min,+).
 * GL_ERR_UNSUPPORTED: what gl_tc_count refuses of a plan, for each of the three (no row copy, num_rows != num_cols, a row shard,
 * entries that do not fit 32-bit offsets, rows that are no strictly ascending sets); plans of different n; nnz(C) >= 2^32. */
int gl_spgemm_symbolic(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask /* may be NULL */, uint32_t flags, uint32_t *d_c_indptr /* n + 1 words */, uint64_t *h_stats /* 4 HOST words, required */);
int gl_spgemm_numeric(gl_spmv_plan a, gl_spmv_plan b, gl_spmv_plan mask, uint32_t flags, uint32_t semiring, const float *d_a_val, const float *d_b_val, const uint32_t *d_c_indptr, uint32_t *d_c_indices, float *d_c_val, uint64_t *h_stats /* may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_SPGEMM_H_ */
