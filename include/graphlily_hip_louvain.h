/*
 * graphlily_hip_louvain.h -- the Louvain extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_louvain.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_LOUVAIN_H_
#define GRAPHLILY_HIP_LOUVAIN_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ONE LEVEL OF LOUVAIN'S LOCAL MOVING over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_louvain.hip), on a
 * square whole-matrix plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is symmetric
 * (io.symmetrize_simple prepares it).  An entry (v, v) is ignored: it is no neighbour, and its weight counts nowhere.  With
 * n = num_rows vertices:
 *   d_weight[j]        = the weight of entry j of the row copy, at least 1, or NULL: every entry weighs 1       (nnz words, read only)
 *   d_vertex_weight[v] = k[v], or NULL: the sum of v's entry weights                                           (n words, read only)
 *   d_color[v]         = a PROPER colouring with colours below n (gl_color gives one)                          (n words, read only)
 *   d_label[v]         = the community of v when the run ends                                                  (n words)
 *   max_sweeps         = the most sweeps to run, at least 1
 *   min_gain           = the smallest growth of Q (below) that a sweep must exceed for the run to go on
 *   h_stats            = {sweeps, moves, evaluations, launches enqueued, stop reason, q_first, q_last}         (7 HOST words, may be NULL;
 *                        the two Q values are signed 64-bit integers in two's complement)
 * THE RULE.  label[v] starts as v.  tot[c] is the sum of k[v] over the members of c.  two_m is the sum of all k[v].  k[v] minus
 * v's entry weights is the vertex's internal weight; it is non-zero on aggregated levels, where self-loops live only here.  A
 * vertex with at least one neighbour is EVALUATED in every sweep (pruning to vertices with a changed neighbour is exact for gl_lpa
 * but not here, because tot moves scores without a neighbour moving).  Evaluating v with own = label[v] computes kin(c), the sum
 * of w(v, u) over neighbours u != v with label[u] == c; cur = two_m * kin(own) - k[v] * (tot[own] - k[v]); for every neighbouring
 * c != own, score(c) = two_m * kin(c) - k[v] * tot[c].  v moves to the SMALLEST c with the largest score(c) if and only if that
 * score is STRICTLY above cur.  All of this is signed 64-bit integer arithmetic; the call requires two_m < 2^31, which keeps every
 * product below 2^62.  A sweep goes class 0, class 1, and so on.  Every vertex of a class decides from the labels AND THE tot
 * ARRAY AS THEY STAND WHEN THE CLASS BEGINS; the class's moves are then applied to label and tot behind a launch boundary, before
 * the next class.  No two vertices of a class are adjacent, so kin is exact; integer adds to tot commute.  Hence labels, sweeps,
 * moves, evaluations and both Q values are properties of (graph, weights, vertex weights, colouring, max_sweeps, min_gain),
 * whatever the schedule of the launches.  Nothing is floating point; two calls give the same bits.
 * Q.  After each sweep, on the device, Q = two_m * In - sum_c tot[c]^2 as a signed 64-bit integer, where In is the sum over v of
 * the internal weight of v plus the sum of w(v, u) over u != v with label[u] == label[v].  Modularity is Q / two_m^2.  q_first is
 * Q of the singletons, q_last Q after the last sweep.
 * THE STOP.  The run stops after the first sweep of these kinds, tested in this order, and reports which as the stop reason:
 * reason 1: the sweep had no move; reason 2: Q_new - Q_old <= min_gain; reason 0: sweep max_sweeps was reached.  Q may fall in a
 * sweep, because scores use the class-start snapshot.  The labels returned are those after the last sweep; what to do with a
 * sweep that lost is the caller's decision.
 * SYMMETRY OF THE WEIGHTS -- d_weight holds the same word in the entries (v, u) and (u, v) -- is the caller's duty and is NOT
 * checked; without it the result is still a pure function of the inputs, but Q is no modularity.
 * d_label is fully written by the call itself, and nothing behind word n is touched.
 * GL_ERR_UNSUPPORTED for a plan without the row copy, with num_rows != num_cols, for a row shard, for rows that are not strictly
 * ascending or hold a column >= num_cols, for a pattern that is not symmetric, and for two_m >= 2^31.  GL_ERR_INVALID_ARG for a
 * NULL plan, d_color or d_label, for max_sweeps == 0, for d_color == d_label, for a colour >= n, for a colouring that is not
 * proper (one launch over the entries finds it; the call says so instead of racing), for a zero entry weight, and for a k[v] below
 * the sum of v's entry weights.  After the last four and the two_m refusal d_label is written, and not a result.  A plan without
 * entries writes own labels and reports {1, 0, 0, launches, 1, 0, 0}.
 * THE CALL SYNCHRONISES: k, tot and Q of the singletons are computed and the vertices bucketed by colour on the device, and the
 * checks' words and the number of classes are read back once; the host then enqueues a fixed batch of sweeps -- per class one
 * launch that decides and one that applies the moves, then one that sums Q and a closing one, every launch gated by a control
 * record on the device --, copies the record to page-locked memory and waits, once per batch, until the record says done.  A
 * plan's first call also establishes the verdicts that the k-core, colouring, k-truss, spanning-forest, matching and label
 * propagation passes cache and allocates 256 + 4 (7 num_rows + 1) bytes of scratch of its own -- the control record, k, tot, the
 * class list, the colour histogram, the class offsets and 2 num_rows words of mover list -- which gl_spmv_plan_destroy frees. */
int gl_louvain_move(gl_spmv_plan plan, const uint32_t *d_weight /* may be NULL: every entry 1 */, const uint32_t *d_vertex_weight /* may be NULL: the sum of the entry weights */, const uint32_t *d_color, uint32_t *d_label, uint32_t max_sweeps, uint64_t min_gain, uint64_t *h_stats /* may be NULL, 7 words: sweeps, moves, evaluations, launches, stop reason, q_first, q_last */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_LOUVAIN_H_ */
