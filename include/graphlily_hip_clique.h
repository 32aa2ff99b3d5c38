/*
 * graphlily_hip_clique.h -- the k-clique counting extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_clique.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_CLIQUE_H_
#define GRAPHLILY_HIP_CLIQUE_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* k-CLIQUE COUNTS over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_clique.hip), gl_tc_count's question
 * for k = 3 .. 8.  N+(x) is row x of the plan, a strictly ascending set of columns; with n = num_rows:
 *   d_total       = the number of sequences (v1, ..., vk) with vj in N+(vi) for every i < j        (one 64-bit word, wrapping)
 *   d_per_vertex  = per[x] = the number of positions that x holds in those sequences      (n 64-bit words, may be NULL)
 *   h_stats       = {rows in the tiny and mid bins, rows in the wide bin, rows in the long bin, launches enqueued}
 *                                                                                          (4 HOST words, may be NULL)
 * A formula about sets, exact whatever the order of the adds: an acyclic orientation (io.orient_by_rank, io.triangle_orient)
 * gives every k-clique once and per[x] = the k-cliques through x, a full symmetric pattern gives every clique k! times, a
 * diagonal entry simply takes part (a vertex that holds two positions of a sequence is counted twice in per[]).  For k = 3
 * both outputs equal gl_tc_count's, to the bit.  Both outputs are zeroed by the call; nothing behind word n of d_per_vertex
 * is touched.  A plan without entries only zeroes its outputs.  Without d_per_vertex the kernels carry no per-vertex
 * bookkeeping.
 * Per source vertex v the call builds the bit matrix of the subgraph induced on N+(v) -- |N+(v)| rows of ceil(|N+(v)| / 32)
 * words, in LDS up to 1024 entries, in a global scratch slab up to 8192 -- and counts the (k - 1)-cliques in it by AND and
 * popcount.  The rows are binned by length at the plan's first call (GRAPHLILY_DEBUG clique_tiny = 32, clique_mid = 256,
 * clique_lds = 1024; clique_lds is the LDS budget, no longer row is staged in LDS) and the bins are cached in the plan.
 * GL_ERR_INVALID_ARG: a NULL plan or d_total, k outside 3 .. 8.
 * GL_ERR_UNSUPPORTED: a plan without the row copy, with num_rows != num_cols, a row shard, entries that do not fit 32-bit
 * offsets, rows that are not strictly ascending sets of columns below num_cols; a row of more than 8192 entries; a long bin
 * whose longest row's matrix does not fit clique_scratch_mb (1024) MiB.  The remedy for the last two is a degeneracy rank:
 * io.orient_by_rank with the positions of KCore.run(order=True) bounds every row by the degeneracy.
 * THE CALL ONLY ENQUEUES, behind the plan's first call (which has the verdict on its rows established, reads the row offsets
 * back once, and allocates the bins -- 4 bytes per row of two entries and more -- and the slabs, all freed by
 * gl_spmv_plan_destroy); h_stats is filled from the cached bins without waiting. */
int gl_clique_count(gl_spmv_plan plan, uint32_t k, uint64_t *d_total, uint64_t *d_per_vertex /* may be NULL: n words */, uint64_t *h_stats /* may be NULL: 4 HOST words: rows per bin {tiny+mid, wide, long}, launches */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_CLIQUE_H_ */
