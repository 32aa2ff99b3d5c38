/*
 * graphlily_hip_match.h -- the greedy-weighted-matching extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_match.hip and nothing else, and capi.EXT_HEADERS maps
 * its file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_MATCH_H_
#define GRAPHLILY_HIP_MATCH_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GREEDY WEIGHTED MATCHING over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_match.hip), on a square
 * whole-matrix plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is symmetric
 * (io.symmetrize_weighted prepares it; the plan is built from all-ones values, because a zero value is stored as column
 * 0xffffffff in the row copy and weight 0 is a legitimate weight).  An ENTRY is a stored (v, u); entry j is word j of the plan's
 * row copy, in the caller's order.  An EDGE is the pair of entries (lo, hi) and (hi, lo), lo < hi; entries (v, v) are no edges.
 * With nnz entries over n = num_cols vertices:
 *   d_weight[j] = the f32 weight of entry j.  Unlike gl_msf, BOTH entries of an edge are read -- each end reads its own row --
 *                 and they must hold the same bits                                                       (nnz words, read only)
 *   d_mate[v]   = the vertex v is matched to, or 0xffffffff if v stays free; d_mate[d_mate[v]] == v      (n words)
 *   h_stats     = {matched edges, rounds, scans, launches enqueued}                                      (4 HOST words, may be NULL)
 *                 rounds = the rounds in which at least one vertex pointed or finished, at most n / 2 + 1; scans = the row
 *                 scans of all rounds together: both are properties of graph and weights, whatever the schedule
 * THE ORDER: edges are ordered by (~key(w), lo, hi), lexicographically and ascending, key(w) = b ^ (b >> 31 ? 0xffffffff :
 * 0x80000000) for the bits b of w -- gl_msf's monotone map of f32 to uint32: the heaviest edge first, and among equal weights the
 * smallest (lo, hi) first.  The order is strict and total.  THE RESULT is the greedy matching in that order: take the edges one by
 * one and keep an edge iff both its ends are still free.  It is unique and maximal, and for non-negative weights its weight is
 * at least half the maximum-weight matching's.  Two calls give the same bits, whatever the schedule.  +-inf are ordinary
 * values; -0.0 sorts below +0.0; a NaN is ordered by its bits (deterministic, with no meaning attached; the drivers refuse NaN
 * and turn -0.0 into +0.0).
 * d_mate is fully written by the call itself.
 * GL_ERR_UNSUPPORTED for a plan without the row copy, with num_rows != num_cols, for a row shard, for rows that are not strictly
 * ascending or hold a column >= num_cols (a zero-valued entry is stored as 0xffffffff), and for a pattern that is not symmetric.
 * A NULL plan, d_weight or d_mate is GL_ERR_INVALID_ARG.  So is a d_weight whose two words of an edge differ in such a way that
 * the vertices' choices close a cycle (0 prefers 1, 1 prefers 2, 2 prefers 0): no pair can form, the result would not be
 * maximal, and the call says so instead (d_mate is then written, and not a result).  A plan without entries (planned in the
 * general layout whatever its flags) writes 0xffffffff to every word of d_mate and reports {0, 0, 0, launches}.
 * THE CALL SYNCHRONISES: it computes the locally dominant matching -- every free vertex points to its best free neighbour, two
 * vertices that point to each other are matched, a vertex whose target was matched elsewhere points again -- which under a
 * strict total order is the greedy matching.  The host enqueues a fixed batch of rounds -- point, match, collect and turn, every
 * launch gated by a control record on the device -- and the closing pass, copies the record to page-locked memory and waits,
 * once per batch, until the record says done (GL_ERR_HIP with the record's contents should that take more than n / 2 + 1 rounds
 * and a batch).  A plan's first call also establishes the verdicts that the k-core, colouring, k-truss and spanning-forest
 * passes cache and allocates 256 + 16 max(num_cols, 1) bytes of scratch -- the control record, a pointer per vertex, two vertex
 * lists and the list of freshly matched vertices -- which gl_spmv_plan_destroy frees. */
int gl_match(gl_spmv_plan plan, const float *d_weight, uint32_t *d_mate, uint64_t *h_stats /* may be NULL, 4 words */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_MATCH_H_ */
