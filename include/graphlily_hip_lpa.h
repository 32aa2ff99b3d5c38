/*
 * graphlily_hip_lpa.h -- the label-propagation extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_lpa.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_LPA_H_
#define GRAPHLILY_HIP_LPA_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LABEL PROPAGATION COMMUNITIES over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_lpa.hip), on a square
 * whole-matrix plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is symmetric
 * (io.symmetrize_simple prepares it).  An entry (v, v) is ignored.  With n = num_rows vertices:
 *   d_color[v]  = a PROPER colouring with colours below n (gl_color gives one), or NULL for the synchronous schedule  (n words, read only)
 *   d_init[v]   = the label v starts with, any word but 0xffffffff, or NULL: v starts with its own number         (n words, read only)
 *   d_label[v]  = the label of v when the run ends                                                               (n words)
 *   max_sweeps  = the most sweeps to run, at least 1
 *   h_stats     = {sweeps, changes, evaluations, launches enqueued, converged}                                   (5 HOST words, may be NULL)
 * THE RULE: label[v] starts as the initial label.  For a vertex v with at least one neighbour, cnt(l) is the number of neighbours
 * carrying l, best = max cnt, cur = cnt(label[v]) (0 if no neighbour carries it).  EVALUATING v: if best > cur, label[v] becomes the
 * SMALLEST l with cnt(l) == best; otherwise it stays -- a tie that includes the current label keeps the current label.
 * COLOUR CLASSES (d_color given): a sweep evaluates class 0, then class 1, and so on, in place.  No two vertices of a class are
 * adjacent, so the result equals a sequential loop over the vertices in (colour, vertex) order.  Every change strictly raises the
 * number of edges whose two ends share a label, so a fixed point is reached.  SYNCHRONOUS (d_color == NULL): a sweep evaluates
 * every vertex from the previous sweep's labels; it may oscillate for ever (a path, a star, any bipartite graph), and max_sweeps
 * ends it.  The run stops after the first sweep that changes nothing (converged = 1) or after max_sweeps sweeps; `sweeps` counts
 * the sweeps run, the empty one included.  A vertex is evaluated in sweep 1 if it has a neighbour, and later iff a neighbour
 * changed since its previous evaluation (synchronous: in the previous sweep) -- evaluating under unchanged neighbour labels
 * changes nothing, so this is exact.  Labels, sweeps, changes, evaluations and converged are properties of (graph, colouring,
 * initial labels, max_sweeps), whatever the schedule of the launches.  Nothing is floating point; two calls give the same bits.
 * d_label is fully written by the call itself, and nothing behind word n is touched.
 * GL_ERR_UNSUPPORTED for a plan without the row copy, with num_rows != num_cols, for a row shard, for rows that are not strictly
 * ascending or hold a column >= num_cols, and for a pattern that is not symmetric.  GL_ERR_INVALID_ARG for a NULL plan or d_label,
 * for max_sweeps == 0, for d_color == d_label, for a label 0xffffffff in d_init (reserved as the empty key of the label tables;
 * found by the pass that copies d_init), for a colour >= n, and for a colouring that is not proper (one launch over the entries
 * finds it; the call says so instead of racing).  After these three d_label is written, and not a result.  A plan without
 * entries writes the initial labels and reports {1, 0, 0, launches, 1}.
 * THE CALL SYNCHRONISES: the vertices are bucketed by colour on the device and the number of classes is read back once; the host
 * then enqueues a fixed batch of sweeps -- one launch per class and a closing one, every launch gated by a control record on the
 * device --, copies the record to page-locked memory and waits, once per batch, until the record says done.  A plan's first call
 * also establishes the verdicts that the k-core, colouring, k-truss, spanning-forest and matching passes cache and allocates
 * 256 + 4 (6 num_rows + 1) bytes of scratch -- the control record, two flag arrays, the second label buffer, the class list,
 * the colour histogram and the class offsets -- which gl_spmv_plan_destroy frees. */
int gl_lpa(gl_spmv_plan plan, const uint32_t *d_color /* may be NULL: synchronous */, const uint32_t *d_init /* may be NULL: own number */, uint32_t *d_label, uint32_t max_sweeps, uint64_t *h_stats /* may be NULL, 5 words: sweeps, changes, evaluations, launches, converged */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_LPA_H_ */
