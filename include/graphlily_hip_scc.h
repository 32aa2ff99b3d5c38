/*
 * graphlily_hip_scc.h -- the strongly-connected-components extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_scc.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_SCC_H_
#define GRAPHLILY_HIP_SCC_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* STRONGLY CONNECTED COMPONENTS over the plain CSR copies two GL_PLAN_BOOLEAN plans keep (gl_scc.hip).  The
 * graph is directed: row v of plan_in lists the PREDECESSORS of v (an edge u -> v for a stored entry A[v, u], as everywhere in
 * this library), row v of plan_out, the plan of the transposed pattern, its SUCCESSORS.  plan_out == plan_in declares a
 * symmetric pattern.  Both are square whole-matrix plans whose rows are strictly ascending sets of columns below num_cols
 * (io.simple_pattern prepares both matrices); an entry (v, v) is ignored.  With n = num_rows vertices:
 *   d_prio[v]   = the priority of v, or NULL: all equal                                                (n words, read only)
 *   d_label[v]  = the SMALLEST vertex u such that v reaches u and u reaches v                           (n words)
 *   h_stats     = {components, passes, trimmed, rounds, launches enqueued}                              (5 HOST words, may be NULL)
 * The labelling is unique -- gl_cc_labels' convention -- and on a symmetric pattern it is gl_cc_labels' result, to the bit.
 * d_prio changes the work, never the labels.
 * THE METHOD: passes of TRIM (a live vertex without a live predecessor or successor is a component of its own; repeated until
 * nothing is removed), FORWARD (every live vertex takes the best key among itself and its live predecessors -- larger priority
 * first, then the smaller vertex, gl_color's order -- to the fixed point: its colour is then the best vertex that reaches it) and
 * BACKWARD (from every vertex that kept its own colour, a root, back along the edges inside its colour class: what is reached is
 * the root's component, which is removed), until no vertex is live.  `passes` counts the passes that reached FORWARD, `trimmed`
 * the vertices TRIM removed: both, like the labels, are properties of (graph, priorities).  `rounds` counts the launches that did
 * a phase's work, the last, empty round of every phase included; it depends on the schedule of the hardware, and is at most the
 * number of synchronous sweeps.  Every pass removes its best live vertex's whole component: hubs first (io.coloring_priorities,
 * "largest_first") normally collects a giant component in pass 1, while a CHAIN of k components whose keys improve along the
 * edges takes k passes.  Nothing is floating point; two calls give the same labels, passes and trimmed.
 * d_label is fully written by the call itself, and nothing behind word n is touched.
 * GL_ERR_UNSUPPORTED, in gl_bc_accumulate's order and wording: a plan without the row copy, with num_rows != num_cols, a row
 * shard, rows that are not strictly ascending (unsorted, or a duplicate column) or hold a zero-valued entry or a column >=
 * num_cols -- for plan_in, then for plan_out --, plans of different sizes, a plan_out that is not the transpose of plan_in
 * (checked on the device on first use and cached in plan_in), and with plan_out == plan_in a pattern that is not symmetric.
 * GL_ERR_INVALID_ARG for a NULL plan or d_label and for d_prio == d_label (d_label holds the state while the call runs).
 * A plan without entries writes label[v] = v in one launch and reports {n, 0, 0, 0, 0}.
 * THE CALL SYNCHRONISES: the host enqueues a fixed batch of (round, turn) launch pairs and the two closing launches -- every
 * launch gated by a control record on the device --, copies the record to page-locked memory and waits, once per batch, until
 * the record says done.  A run that exceeds n^2 + 6 n + 8 steps, or a batch that leaves the record as it was, ends with
 * GL_ERR_HIP ("internal error") instead of hanging.  plan_in's first call also establishes the verdicts named above and
 * allocates 256 + 24 num_rows bytes of scratch -- the control record, a 64-bit colour word per vertex, the marks, the
 * components' minima and two lists of live vertices -- which gl_spmv_plan_destroy frees. */
int gl_scc(gl_spmv_plan plan_in, gl_spmv_plan plan_out /* == plan_in: symmetric */, const uint32_t *d_prio /* may be NULL: all equal */, uint32_t *d_label, uint64_t *h_stats /* may be NULL, 5 words: components, passes, trimmed, rounds, launches */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_SCC_H_ */
