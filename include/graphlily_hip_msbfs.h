/*
 * graphlily_hip_msbfs.h -- the multi-source breadth-first-search extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_msbfs.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_MSBFS_H_
#define GRAPHLILY_HIP_MSBFS_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* BIT-PARALLEL MULTI-SOURCE BFS over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_msbfs.hip; Then et al.,
 * VLDB 2014): the hop distances from k <= 64 sources in ONE sweep, every vertex holding a 64-bit word with one bit per source.
 * The graph is directed: row v of the plan lists the PREDECESSORS of v (an edge u -> v for a stored entry A[v, u], as everywhere
 * in this library), so the call measures d(s, v), the edges of a shortest path FROM source s TO v; the transposed pattern's plan
 * gives the distances to the sources.  A column 0xffffffff (a zero-valued entry) is no edge, a diagonal entry is harmless; the
 * rows need be neither sorted nor sets nor symmetric.  With n = num_rows vertices:
 *   h_sources     = k vertices below n, k in 1 .. 64; a vertex given twice occupies two bits and counts twice  (k HOST words)
 *   d_far[v]      = the sum of d(s, v) over the sources with 1 <= d(s, v) < inf                               (n 64-bit words)
 *   d_reach[v]    = the number of those sources                                                                (n words)
 *   d_harmonic[v] = the f64 sum of (double)c / (double)d in a FIXED order: the levels d = 1, 2, ... ascending, c = the sources
 *                   that reach v at level d, one division and one addition per level with c > 0              (n doubles)
 *   accumulate    = 0: the call initialises the three arrays; otherwise it adds to them -- integer adds, and the harmonic sum
 *                   goes on in the same order -- so after a driver's batches far and reach are functions of (graph, source
 *                   multiset) and harmonic of (graph, source SEQUENCE)
 *   d_hops[j n + v] = d(h_sources[j], v): 0 on the source itself, 0xffffffff when unreached; every one of the k n words is
 *                   written by the call                                                                  (k n words, may be NULL)
 *   h_source_stats[3 j ..] = {vertices at distance >= 1 from source j, the sum of those distances, the eccentricity: the
 *                   largest finite distance}                                                       (3 k HOST words, may be NULL)
 *   h_stats       = {levels swept: the largest eccentricity, vertices that have met all k sources (distance 0 included),
 *                   launches enqueued, 0}                                                            (4 HOST words, may be NULL)
 * Everything but `launches` is a function of the arguments, whatever the schedule: every vertex has ONE writer, no word of a
 * vertex is touched by an atomic, and there is no floating-point atomic anywhere.  Nothing behind word n (k n of d_hops) is
 * touched.
 * GL_ERR_UNSUPPORTED: a plan without the row copy, with num_rows != num_cols, a row shard, entries that do not fit 32-bit offsets.
 * GL_ERR_INVALID_ARG: a NULL plan or h_sources, a NULL d_far, d_reach or d_harmonic, k outside 1 .. 64, a source >= n (which
 * includes every call on a plan with n == 0: no source can be named), and output arrays that overlap.
 * A plan without entries answers from one launch: everything is 0, hops is 0 on each source's own vertex and 0xffffffff elsewhere.
 * THE CALL SYNCHRONISES: the host enqueues a fixed batch of level launches -- each gated by a control word on the device: it
 * returns at once when the level before it added no bit --, copies the control words to page-locked memory and waits, once per
 * batch, until they say done.  A run that exceeds n + 1 steps ends with GL_ERR_HIP ("internal error") instead of hanging.
 * The plan's first call allocates 1536 + 24 num_rows bytes of scratch -- 256 bytes of control record, the per-source counters,
 * the seen words and the two frontiers -- which gl_spmv_plan_destroy frees. */
int gl_msbfs(gl_spmv_plan plan, const uint32_t *h_sources, uint32_t k /* 1 .. 64 */, int accumulate, uint64_t *d_far, uint32_t *d_reach, double *d_harmonic, uint32_t *d_hops /* may be NULL: k * n words */, uint64_t *h_source_stats /* may be NULL: 3 * k HOST words */, uint64_t *h_stats /* may be NULL: 4 HOST words */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_MSBFS_H_ */
