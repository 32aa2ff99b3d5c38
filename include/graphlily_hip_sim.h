/*
 * graphlily_hip_sim.h -- the neighbourhood-similarity extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_sim.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_SIM_H_
#define GRAPHLILY_HIP_SIM_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* COMMON NEIGHBOURS OF CALLER-CHOSEN PAIRS over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_sim.hip):
 * what the Jaccard, overlap, Sorensen and cosine coefficients, the Adamic-Adar and the resource-allocation index are functions
 * of.  N(x) is row x of the plan, a strictly ascending set of columns; with n = num_rows:
 *   d_pairs         = u0 v0 u1 v1 ...: m pairs of vertices, which need not be edges                            (2 m words)
 *   d_common[i]     = |N(u_i) & N(v_i)|                                                                         (m words)
 *   d_vertex_weight = a 64-bit unsigned weight per vertex                                          (n 64-bit words, may be NULL)
 *   d_weighted[i]   = the sum of d_vertex_weight[w] over the w of N(u_i) & N(v_i), in 64-bit unsigned integers WRAPPING modulo
 *                     2^64: integer adds commute, so any reduction tree gives the same bits; real weights are the caller's
 *                     fixed point                                       (m 64-bit words, may be NULL; needs d_vertex_weight)
 *   h_stats         = {pairs out of range, pairs that took the deferred (long) path, launches enqueued, 0}
 *                                                                                                (4 HOST words, may be NULL)
 * u == v is legal and gives the whole row; (u, v) and (v, u) give the same words; a pair given twice is computed twice.  A
 * pair with u >= n or v >= n gets d_common = 0xffffffff and d_weighted = 0 and is counted in h_stats[0].  Every output word has
 * ONE writer, no atomic touches an output and there is no floating-point operation anywhere: everything but `launches` is a
 * function of the arguments, whatever the schedule.  Nothing behind word m of either output is touched.
 * Symmetry is NOT required: on a directed pattern (row v: the predecessors of v) the call counts common predecessors, and the
 * transposed pattern's plan gives common successors.
 * m == 0 is GL_OK and writes nothing.  A plan without entries answers every in-range pair with 0 from one launch.
 * GL_ERR_UNSUPPORTED: a plan without the row copy, with num_rows != num_cols, a row shard, entries that do not fit 32-bit
 * offsets, rows that are not strictly ascending sets of columns below num_cols (io.symmetrize_simple and io.simple_pattern
 * prepare such a matrix).
 * GL_ERR_INVALID_ARG: a NULL plan, a NULL d_pairs or d_common with m > 0, d_weighted without d_vertex_weight, m above 2^32 - 1,
 * outputs that overlap each other or the pairs.
 * WITHOUT h_stats THE CALL ONLY ENQUEUES (behind the plan's first call, which has the verdict on its rows established and
 * allocates the scratch); with h_stats it synchronises once to read the two counters back.  The pairs are taken in chunks of
 * at most 2^20, two launches each: the first answers the pairs whose shorter row has at most sim_short entries and appends the
 * others to a list, the second -- which reads the list's length on the device -- answers those with a wavefront per pair.
 * The plan's first call allocates 256 + 4 Mi bytes of scratch -- the control record and the list -- which gl_spmv_plan_destroy
 * frees. */
int gl_similarity(gl_spmv_plan plan, const uint32_t *d_pairs /* 2 m words: u0 v0 u1 v1 ... */, uint64_t m, const uint64_t *d_vertex_weight /* may be NULL: n words */, uint32_t *d_common /* m words */, uint64_t *d_weighted /* may be NULL: m words */, uint64_t *h_stats /* may be NULL: 4 HOST words */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_SIM_H_ */
