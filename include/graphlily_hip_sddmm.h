/*
 * graphlily_hip_sddmm.h -- the sampled dense x dense product extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_sddmm.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the name it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_SDDMM_H_
#define GRAPHLILY_HIP_SDDMM_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SDDMM, the product of two dense blocks sampled at the entries of a sparse pattern (gl_sddmm.hip):
 *
 *   out[e] = a_e (x) ( zero (+) sum over c in [0, k) of  X[r, c] (x) Y[j, c] )
 *            for every entry e = (r, j) of rows [row_begin, row_end) of the plan's row copy, in the copy's order
 *
 * -- C<A> = X (+).(x) Y^T kept at A's entries only; the score of every edge from the features of its two end points.  `op` is
 * a gl_op, `zero` the semiring's zero as in gl_spmv_run:
 *   GL_OP_MULADD   a (zero + sum of x y)
 *   GL_OP_ADDMIN   a + min(zero, min over c of (x + y))
 *   GL_OP_ANDOR    1.0 where some c has X != 0 and Y != 0, else `zero`; no value of A is read
 * X is num_rows x k floats, row-major, with the leading dimension ldx >= k (element (r, c) is d_x[r ldx + c], r the GLOBAL row
 * number, also for a row shard); Y is num_cols x k with ldy; the offsets into both are 64-bit.
 *
 * THE MATRIX is a GL_PLAN_BOOLEAN plan of all-ones values, read through its plain row copy, as gl_spmm reads it: it may be
 * rectangular and a row shard, its rows need be neither sorted nor sets (an entry stored twice gets two results).  d_out holds
 * one f32 per entry of the row copy (of the shard's part of it, for a row shard), in the caller's order, and d_a_val, when it is
 * not NULL, one value per entry by the same numbering -- the convention of d_a_val in gl_spmm, gl_spgemm_numeric, gl_msf and
 * gl_sssp_delta, so that d_out can be handed to any of them as it is.  A NULL d_a_val means no scaling: the bracket itself.
 * AN ENTRY WHOSE STORED COLUMN IS 0xffffffff -- what the row copy keeps of an entry the plan was created with a zero value for --
 * OR IS NOT BELOW num_cols WRITES THE LITERAL 0 AT ITS PLACE under every semiring, whatever d_a_val holds there.  Only the
 * entries' words of d_out are written.  A plan without entries writes nothing and succeeds.
 *
 * ARITHMETIC.  (+,x): every product, the whole sum over the k features, the addition of `zero` and the scaling by a are formed
 * in f64 -- the product of two f32 values is exact in f64 -- and rounded to f32 ONCE, at the store; no floating-point atomic is
 * used.  The order of the sum depends ONLY ON k: not on the path, the row's length, the entry's place in its row, nor on
 * whether the 16-byte loads or their dword twin ran; so two calls, two paths and two load widths all give the same bits.  So
 * |out - exact| <= 2^-24 |exact| + (k + 1) 2^-52 |a| sum|x y| + 2^-149  (k + 2 with a non-zero `zero`).  (min,+): x + y in f32,
 * then the minimum over c and with `zero`, then + a in f32: independent of the order, to be compared for equality.  (||,&&):
 * exact.  The library reads the values as they are; the module layer refuses NaN under every semiring and +-inf under (+,x).
 *
 * HOW.  A wavefront is G groups of W lanes, G W = 64; a lane owns four consecutive features of every tile of 4 W; W = 1, 4, 16,
 * 64 for k <= 4, 16, 64 and above, and for k > 256 a lane strides over the 256-feature tiles itself.  The group's partial sums
 * meet by shuffles at the distances 1 ... W / 2.  A lane loads 16 bytes at a time when the bases and leading dimensions allow
 * it; the dword twin serves the rest (GRAPHLILY_DEBUG sddmm_vec=0 forces it).  X's row is loaded ONCE per row (or piece) and
 * kept in registers up to k = 1024; above, the workgroup stages it in LDS (up to 64 KiB, k = 16384; beyond that the lanes read
 * it through the cache).  Two paths by a row's entry count: up to sddmm_cut (32) a group per row; above, the row is cut into
 * pieces of sddmm_piece (256, rounded up to a multiple of 64) entries and a wavefront takes a piece: it loads 64 columns
 * coalesced, hands them to its groups by shuffles and stores 64 results coalesced.  sddmm_short=0 sends every row to the piece
 * path.  The two lists come from one counting pass on the plan's first call, which waits once; they are cached in the plan,
 * keyed by the two knobs and not by k, and rebuilt when a call reads other knobs.  The defaults are starting values.
 *
 * h_stats (3 HOST words, may be NULL; when given, the call WAITS) = {rows on the short path, pieces on the piece path, feature
 * tiles}.  Otherwise the call only enqueues (the plan's first call excepted).
 *
 * GL_ERR_INVALID_ARG: a NULL plan, d_x, d_y or d_out (a NULL d_out is allowed for a plan without entries); k == 0; ldx or ldy
 * below k; an op that is no gl_op; d_out's byte range overlapping X's, Y's or d_a_val's.  GL_ERR_UNSUPPORTED: a plan with
 * entries but no row copy; entries that do not fit 32-bit offsets. */
int gl_sddmm(gl_spmv_plan plan, const float *d_a_val /* may be NULL: no scaling */, const float *d_x, uint64_t ldx, const float *d_y, uint64_t ldy, float *d_out, uint32_t k, int op, float zero, uint64_t *h_stats /* 3 HOST words, may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_SDDMM_H_ */
