/*
 * graphlily_hip_ext.h -- extensions to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * THE FIRST EXTENSION HEADER; LATER EXTENSIONS GET A HEADER OF THEIR OWN (graphlily_hip_truss.h is the next; capi.EXT_HEADERS
 * lists them all).  graphlily_hip.h is the drop-in boundary of the reference's operator API plus the graph kernels that grew next
 * to it, and its list of entry points is pinned by tests that stay as they are (the CPU suite compares it with capi.EXPORTS, name
 * by name and by count); this header's list, capi.EXT_EXPORTS, has been pinned in the same way since.  The colouring entry point
 * below is declared here and named in capi.EXT_EXPORTS, which the suite and the build check against this header and the library.  The
 * conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are device
 * pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_EXT_H_
#define GRAPHLILY_HIP_EXT_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GRAPH COLOURING over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_color.hip), on a square whole-matrix
 * plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is symmetric (io.symmetrize_simple
 * prepares it); an entry (v, v) is ignored.  n = num_rows:
 *   d_prio      = n priorities, or NULL: every priority 0.  u GOES BEFORE v iff d_prio[u] > d_prio[v], or they are equal and
 *                 u < v -- a total order; NULL is plain ascending vertex order                              (n words, read only)
 *   d_color[v]  = the smallest non-negative integer that is not the colour of a neighbour going before v: sequential first-fit
 *                 greedy in that order.  A pure function of (graph, d_prio): two calls give the same bits.  Isolated vertices
 *                 get 0, every colour is at most the degree                                                 (n words)
 *   h_stats     = {num_colors = max colour + 1, rounds, launches enqueued, widest}                          (4 HOST words, may be NULL)
 *                 round[v] = 1 + max round[u] over the neighbours u going before v (1 without any); rounds = max round, the
 *                 depth of the priority order's DAG; widest = the largest number of vertices sharing a round
 * Jones-Plassmann colouring with dependency counters: d_color itself holds, while v is uncoloured, the number of its neighbours
 * that go before it and are uncoloured; a device-resident queue receives v when that count reaches 0; one launch per round
 * colours a slice of the queue and decrements the counts behind it, each launch gated by a control record on the device, so the
 * result does not depend on how many launches are enqueued at a time.  Every vertex is visited once, every stored entry once by
 * the count and once by the round of its row (hub rows whose colour is 256 or more are re-read once per further 256 colours).
 * d_color is fully written by the call itself.
 * GL_ERR_UNSUPPORTED for a plan without the row copy, with num_rows != num_cols, for a row shard (row u must be readable for
 * every column u), for rows that are not strictly ascending or hold a column >= num_cols (a zero-valued entry is stored as
 * 0xffffffff), and for a pattern that is not symmetric.  A NULL plan or d_color, or d_prio == d_color, is GL_ERR_INVALID_ARG.
 * With n == 0 nothing is written and h_stats is zero.  A plan without entries (planned in the general layout whatever its flags)
 * is an empty graph: d_color zero, h_stats {1, 1, 0, n}.
 * THE CALL SYNCHRONISES: the host enqueues a fixed batch of gated launches, copies the control record to page-locked memory and
 * waits, once per batch, until the record says done (at most n rounds exist; GL_ERR_HIP should the cap ever be hit).  A plan's
 * first call also establishes the verdicts gl_kcore caches (the rows are such sets, the pattern is symmetric) and allocates
 * 256 + 4 n bytes of scratch, which gl_spmv_plan_destroy frees. */
int gl_color(gl_spmv_plan plan, const uint32_t *d_prio /* may be NULL */, uint32_t *d_color, uint64_t *h_stats /* may be NULL, 4 words: num_colors, rounds, launches, widest */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_EXT_H_ */
