/*
 * graphlily_hip_sssp_delta.h -- the delta-stepping shortest-paths extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_sssp_delta.hip and nothing else, and capi.EXT_HEADERS maps
 * its file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_SSSP_DELTA_H_
#define GRAPHLILY_HIP_SSSP_DELTA_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SHORTEST PATHS BY DELTA-STEPPING (Meyer and Sanders), run to convergence on the device, over the plain CSR copies two
 * GL_PLAN_BOOLEAN plans keep (gl_sssp_delta.hip).  The graph is directed: row v of plan_in lists the PREDECESSORS
 * of v (an edge u -> v for a stored entry A[v, u], as everywhere in this library), row u of plan_out, the plan of the transposed
 * pattern, its SUCCESSORS.  plan_out == plan_in declares a symmetric pattern; the two weight arrays may still differ.  Both are
 * square whole-matrix plans whose rows are strictly ascending sets of columns below num_cols (io.directed_weighted prepares both
 * matrices and both weight arrays); an entry (v, v) is harmless.  With n = num_rows vertices:
 *   d_weight_in[j]  = the f32 weight of entry j of plan_in's row copy, d_weight_out[j] that of entry j of plan_out's: FINITE,
 *                     >= +0.0 and not -0.0 (the drivers refuse the rest; the call does not check)      (nnz words each, read only)
 *   d_sources       = num_sources vertex numbers, all at distance 0; a number >= n is ignored, one given twice counts once
 *   delta           = the bucket width: a finite f32 > 0, or +inf -- one bucket, no heavy edge: frontier Bellman-Ford
 *   d_dist[v]       = the least fixed point of d[s] = +0.0 for every source and d[v] = min over the stored entries A[v, u] of
 *                     (float)(d[u] + w), in f32 arithmetic: what Dijkstra's algorithm computes in f32, to the bit, whatever
 *                     delta, the schedule and the knobs.  A sum may overflow to +inf: such a vertex counts as unreached.
 *                     Unreached vertices hold the bits 0x7f800000                                                      (n words)
 *   d_parent[v]     = v for a source; 0xffffffff for an unreached vertex; otherwise the SMALLEST u with a stored A[v, u], d[u] <
 *                     d[v] and (float)(d[u] + w) == d[v] (SSSP.parents()'s definition), from one final pull pass over plan_in in
 *                     which every vertex has one writer.  A reached vertex that is no source and has no such u -- an ORPHAN, which
 *                     exists only behind zero-weight edges -- keeps 0xffffffff                          (n words, may be NULL)
 *   h_stats         = {reached, buckets visited, rounds, relaxations that lowered a distance, launches enqueued}
 *                                                                                                  (5 HOST words, may be NULL)
 * `reached` (the vertices with a finite distance) is a function of the input.  The other four depend on the order in which the
 * hardware serves the atomics of a launch -- a round may carry a distance one edge or several -- and on the knobs: they are
 * diagnostics, and nothing may be pinned to them.  (With delta = +inf `buckets visited` is 1 whenever a source is a vertex.)
 * Every output word is written by the call itself, and nothing behind word n is touched.
 * GL_ERR_UNSUPPORTED, in gl_topo's order and wording: a plan without the row copy, with num_rows != num_cols, a row shard, rows
 * that are not strictly ascending or hold a zero-valued entry or a column >= num_cols -- for plan_in, then for plan_out --, plans
 * of different sizes, a plan_out that is not the transpose of plan_in, and with plan_out == plan_in a pattern that is not symmetric.
 * GL_ERR_INVALID_ARG for a NULL plan, weight array or d_dist, a NULL d_sources with num_sources > 0, a delta that is <= 0 or NaN,
 * and arrays that overlap.
 * A plan without entries, or num_sources == 0, is answered in ONE launch (which looks every vertex up in the list of sources)
 * and reports {reached, 0, 0, 0, 1}; n == 0 reports zeros.
 * THE CALL SYNCHRONISES: the host enqueues a fixed batch of steps -- every launch gated by a control record on the device --,
 * copies the record to page-locked memory and waits, once per batch, until the record says done.  A run takes at most 2 n + 1
 * steps where every heavy edge leaves its bucket, and at most n (n + 1) + 1 where some stay in it (the clamped top bucket, a delta
 * below f32's spacing); one that exceeds n (n + 1) + 4 steps, or a batch that leaves the record as it was, ends with GL_ERR_HIP
 * ("internal error") instead of hanging.
 * plan_in's first call also establishes the verdicts named above and allocates 256 + 36 num_rows bytes of scratch, which
 * gl_spmv_plan_destroy frees: nothing is O(nnz), and no list can overflow. */
int gl_sssp_delta(gl_spmv_plan plan_in, gl_spmv_plan plan_out /* == plan_in: symmetric */, const float *d_weight_in, const float *d_weight_out, const uint32_t *d_sources, uint32_t num_sources, float delta, float *d_dist, uint32_t *d_parent /* may be NULL */, uint64_t *h_stats /* may be NULL, 5 words: reached, buckets, rounds, relaxations, launches */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_SSSP_DELTA_H_ */
