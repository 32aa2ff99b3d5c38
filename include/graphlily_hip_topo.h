/*
 * graphlily_hip_topo.h -- the topological-levels extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_topo.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_TOPO_H_
#define GRAPHLILY_HIP_TOPO_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TOPOLOGICAL LEVELS AND CRITICAL PATHS over the plain CSR copies two GL_PLAN_BOOLEAN plans keep (gl_topo.hip).
 * The graph is directed: row v of plan_in lists the PREDECESSORS of v (an edge u -> v for a stored entry A[v, u], as everywhere in
 * this library), row v of plan_out, the plan of the transposed pattern, its SUCCESSORS.  plan_out == plan_in declares a
 * symmetric pattern.  Both are square whole-matrix plans whose rows are strictly ascending sets of columns below num_cols
 * (io.directed_weighted and io.simple_pattern prepare both matrices); an entry (v, v) is ignored.  With n = num_rows vertices:
 *   d_weight[j] = the f32 weight of entry j of plan_in's row copy: FINITE and not -0.0 (the drivers refuse NaN and +-inf and
 *                 store -0.0 as +0.0; the call does not check), or NULL: unweighted                     (nnz words, read only)
 *   d_level[v]  = the number of edges of the longest path that ends in v: 0 for a vertex without predecessors, else 1 + the
 *                 largest level of a predecessor; 0xffffffff for a vertex on a cycle or reachable from one   (n words)
 *   d_order     = the queue: the peeled vertices grouped by ascending level -- the order inside a level is UNSPECIFIED --, then
 *                 0xffffffff in every remaining word                                                      (n words, may be NULL)
 *   d_dist[v]   = +0.0f for a peeled vertex without predecessors, else the largest, under > on float, of (float)(dist[u] +
 *                 w(u, v)) over the predecessors u, in f32 arithmetic; the bits 0x7fc00000 for an unpeeled vertex.  Sums may
 *                 overflow to +-inf; no dist is NaN or -0.0                                     (n words, given iff d_weight is)
 *   d_parent[v] = the SMALLEST u that attains dist[v]; 0xffffffff for sources and unpeeled vertices (n words, given iff d_weight is)
 *   h_stats     = {peeled, levels, widest, launches enqueued}                                         (4 HOST words, may be NULL)
 * `levels` counts the non-empty levels -- 1 + the edges of the longest path --, `widest` is the largest level's size; level,
 * dist, parent and the first three stats are functions of (graph, weights), whatever the schedule: every vertex has ONE writer,
 * which reduces the 64-bit word key(dist[u] + w) << 32 | ~u over its row by max -- no float atomic, no spin-wait.  peeled < n is
 * a RESULT: the graph has a cycle, and the unpeeled vertices are those on a cycle or behind one.
 * HEIGHTS (the longest path to a sink) and a latest-start pass are the same call with the two plans swapped and the weights
 * aligned with plan_out's entries; the longest path under NEGATED weights is the shortest path of the DAG.
 * Every output word is written by the call itself, and nothing behind word n is touched.
 * GL_ERR_UNSUPPORTED, in gl_scc's order and wording: a plan without the row copy, with num_rows != num_cols, a row shard, rows
 * that are not strictly ascending (unsorted, or a duplicate column) or hold a zero-valued entry or a column >= num_cols -- for
 * plan_in, then for plan_out --, plans of different sizes, a plan_out that is not the transpose of plan_in (checked on the
 * device on first use and cached in plan_in), and with plan_out == plan_in a pattern that is not symmetric.
 * GL_ERR_INVALID_ARG for a NULL plan or d_level, d_dist or d_parent without d_weight (or the reverse), and arrays that overlap.
 * A plan without entries writes level = 0 everywhere (order = 0 .. n - 1, dist = +0, parent = 0xffffffff) in one launch and
 * reports {n, 1, n, 1}; n == 0 reports {0, 0, 0, 0}.
 * THE CALL SYNCHRONISES: the host enqueues a fixed batch of (round, turn) launch pairs -- every launch gated by a control record
 * on the device --, copies the record to page-locked memory and waits, once per batch, until the record says done.  A run that
 * exceeds n + 1 steps, or a batch that leaves the record as it was, ends with GL_ERR_HIP ("internal error") instead of hanging.
 * plan_in's first call also establishes the verdicts named above and allocates 256 + 8 num_rows bytes of scratch -- the control
 * record, the dependency counters and the queue -- which gl_spmv_plan_destroy frees. */
int gl_topo(gl_spmv_plan plan_in, gl_spmv_plan plan_out /* == plan_in: symmetric */, const float *d_weight /* may be NULL: unweighted */, uint32_t *d_level, uint32_t *d_order /* may be NULL */, float *d_dist /* given iff d_weight is */, uint32_t *d_parent /* given iff d_weight is */, uint64_t *h_stats /* may be NULL, 4 words: peeled, levels, widest, launches */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_TOPO_H_ */
