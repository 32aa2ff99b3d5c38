/*
 * graphlily_hip_msf.h -- the minimum-spanning-forest extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_msf.hip and nothing else, and capi.EXT_HEADERS maps
 * its file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_MSF_H_
#define GRAPHLILY_HIP_MSF_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MINIMUM SPANNING FOREST over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_msf.hip), on a square
 * whole-matrix plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is symmetric
 * (io.symmetrize_weighted prepares it; the plan is built from all-ones values, because a zero value is stored as column
 * 0xffffffff in the row copy and weight 0 is a legitimate weight).  An ENTRY is a stored (v, u); entry j is word j of the plan's
 * row copy, in the caller's order.  An EDGE is the pair of entries (lo, hi) and (hi, lo), lo < hi; entries (v, v) are no edges.
 * With nnz entries over n = num_cols vertices:
 *   d_weight[j]    = the f32 weight of entry j.  The weight of edge {lo, hi} is the word of the entry ABOVE the diagonal,
 *                    (lo, hi); the word of the mirror entry is never read                                  (nnz words, read only)
 *   d_in_forest[j] = 1 if the edge of entry j is in the forest, 0 otherwise; both entries of an edge carry the same value,
 *                    an entry (v, v) gets 0                                                                 (nnz words)
 *   d_labels[v]    = the smallest vertex of v's component: bit-equal to gl_cc_labels on the same plan       (n words, may be NULL)
 *   h_stats        = {forest edges, components over the n vertices, rounds, launches enqueued}              (4 HOST words, may be NULL)
 *                    forest edges + components == n; rounds = the Boruvka rounds in which at least one component chose an
 *                    edge, at most ceil(log2 n): a property of graph and weights (every component chooses in every round)
 * THE ORDER: edges are ordered by (key(w), lo, hi), lexicographically, key(w) = b ^ (b >> 31 ? 0xffffffff : 0x80000000) for the
 * bits b of w -- the monotone map of f32 to uint32.  The order is strict and total, so the minimum spanning forest under it is
 * unique: the one Kruskal's algorithm returns when it takes the edges in this order.  That forest is the result, whatever the
 * schedule: two calls give the same bits.  +-inf are ordinary values; -0.0 sorts below +0.0; a NaN is ordered by its bits
 * (deterministic, with no meaning attached; the drivers refuse NaN and turn -0.0 into +0.0).
 * d_in_forest is fully written by the call itself, and so is d_labels.
 * GL_ERR_UNSUPPORTED for a plan without the row copy, with num_rows != num_cols, for a row shard, for rows that are not strictly
 * ascending or hold a column >= num_cols (a zero-valued entry is stored as 0xffffffff), and for a pattern that is not symmetric.
 * A NULL plan, d_weight or d_in_forest, or d_labels == d_in_forest, is GL_ERR_INVALID_ARG.  A plan without entries (planned in
 * the general layout whatever its flags) writes no forest words, labels every vertex with itself and reports {0, n, 0, launches}.
 * THE CALL SYNCHRONISES: the host enqueues a fixed batch of rounds -- scan, hook, turn and ceil(log2 n) + 1 pointer-doubling
 * steps each, every launch gated by a control record on the device -- and the closing passes, copies the record to page-locked
 * memory and waits, once per batch, until the record says done (GL_ERR_HIP with the record's contents should that take more than
 * ceil(log2 n) + 1 rounds and a batch).  A plan's first call also establishes the verdicts that the k-core, colouring and
 * k-truss passes cache and allocates 256 + 28 max(num_cols, 1) bytes of scratch -- the control record, a 64-bit best-edge word
 * per vertex, two component arrays, the rows' first entries above the diagonal and the list of forest edges -- which
 * gl_spmv_plan_destroy frees. */
int gl_msf(gl_spmv_plan plan, const float *d_weight, uint32_t *d_in_forest, uint32_t *d_labels /* may be NULL */, uint64_t *h_stats /* may be NULL, 4 words */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_MSF_H_ */
