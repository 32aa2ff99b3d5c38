/*
 * graphlily_hip_spmm.h -- the sparse matrix x dense block extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_spmm.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the name it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_SPMM_H_
#define GRAPHLILY_HIP_SPMM_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SpMM, the product of a sparse matrix with a dense block of k vectors (gl_spmm.hip):
 *
 *   Y[r, c] = mask(r, c) ? ( zero (+) sum over the entries (r, j) of A of  A_rj (x) X[j, c] ) : 0
 *             for r in [row_begin, row_end) of the plan, c in [0, k)
 *
 * `op` is a gl_op (GL_OP_MULADD, GL_OP_ANDOR, GL_OP_ADDMIN), `zero` the semiring's zero as in gl_spmv_run, `mask_type` a
 * gl_mask.  The mask is a dense f32 block of Y's shape, read per element exactly as gl_spmv_run reads its mask per row:
 * GL_MASK_WRITETOZERO keeps the elements whose mask == 0, GL_MASK_WRITETOONE those whose mask != 0; a masked-off element is
 * written as the literal 0.  X is num_cols x k floats, row-major, with the leading dimension ldx >= k (element (j, c) is
 * d_x[j ldx + c]); Y is num_rows x k with ldy, the mask num_rows x k with ldm; the offsets into all three are 64-bit.  Rows
 * [row_begin, row_end) of Y are written, their k columns each, and nothing else: not the words between k and ldy, no other row.
 *
 * THE MATRIX is a GL_PLAN_BOOLEAN plan of all-ones values, read through its plain row copy; the values travel apart from the
 * plan: d_a_val[j] is the f32 value of entry j of the row copy (of the shard's part of it, for a row shard), in the caller's
 * order -- the convention of gl_spgemm_numeric, gl_msf and gl_sssp_delta; a zero VALUE is a value here.  Nothing more is
 * required of the plan: it may be rectangular, its rows need be neither sorted nor sets (an entry stored twice counts twice), and
 * a row shard is served.  AN ENTRY WHOSE STORED COLUMN IS 0xffffffff -- what the row copy keeps of an entry the plan was created
 * with a zero value for -- IS SKIPPED UNDER EVERY SEMIRING, whatever d_a_val holds at its place.  A plan without entries keeps no
 * row copy and is served all the same: one launch writes mask ? zero : 0.
 *
 * ARITHMETIC.  (+,x): every product and the whole row sum are formed in f64 -- the product of two f32 values is exact in f64 --
 * and rounded to f32 ONCE, at the store; no floating-point atomic is used; the order of a row's sum depends only on the row, k
 * and the path, so two calls give the same bits.  So |y - exact| <= 2^-24 |exact| + p 2^-52 sum|a x| + 2^-149 for a row of p
 * entries.  (min,+): a + x in f32, then the minimum with `zero`: independent of the order.  (||,&&): no value is read and
 * d_a_val may be NULL; the result is 1.0 where some entry of the row meets an X != 0, else `zero`.  The library reads the
 * values as they are; the module layer refuses NaN under every semiring and +-inf under (+,x).
 *
 * HOW.  A wavefront is G groups of W lanes, G W = 64; a lane owns four consecutive columns, a group a tile of 4 W columns; W =
 * 1, 4, 16, 64 for k <= 4, 16, 64 and above, and k > 256 takes tiles of 256 columns on the grid's second dimension, each of
 * which re-walks the row.  A lane loads 16 bytes of X per entry when the bases, ldx, ldy (and ldm) allow it; the dword twin
 * serves unaligned bases, leading dimensions that are no multiple of 4 and the ragged last tile (GRAPHLILY_DEBUG spmm_vec=0
 * forces it).  Three paths per row by its entry count: up to spmm_cut (32) a group per row, G rows per wavefront step; up to
 * spmm_wg (4096) a wavefront per row, which loads columns and values coalesced and hands them to the groups by shuffles, the
 * groups' sums meeting by shuffles in a fixed order; above, the four wavefronts of a workgroup share one row and add their f64
 * tiles through LDS in wavefront order.  spmm_short=0 / spmm_wave=0 close the first / the second path (their rows take the
 * next).  The row lists per path come from one counting pass on the plan's first call, which reads the knobs and waits once;
 * they are cached in the plan, keyed by the two cuts and not by k.  The defaults are starting values.
 *
 * h_stats (4 HOST words, may be NULL; when given, the call WAITS) = {rows on the short path, rows on the wavefront path, rows
 * on the workgroup path, column tiles}.  Otherwise the call only enqueues (the plan's first call excepted).
 *
 * GL_ERR_INVALID_ARG: a NULL plan, d_x or d_y; k == 0; ldx or ldy below k; a mask_type that is no gl_mask; with a mask type a
 * NULL d_mask or ldm below k; an op that is no gl_op; a NULL d_a_val unless GL_OP_ANDOR; Y's byte range overlapping X's or the
 * mask's.  GL_ERR_UNSUPPORTED: a plan with entries but no row copy; entries that do not fit 32-bit offsets. */
int gl_spmm(gl_spmv_plan plan, const float *d_a_val /* may be NULL under GL_OP_ANDOR */, const float *d_x, uint64_t ldx, const float *d_mask /* NULL without a mask */, uint64_t ldm, float *d_y, uint64_t ldy, uint32_t k, int op, float zero, int mask_type, uint64_t *h_stats /* 4 HOST words, may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_SPMM_H_ */
