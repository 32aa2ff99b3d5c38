/*
 * graphlily_hip_truss.h -- the k-truss extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_truss.hip and nothing else, and capi.EXT_HEADERS maps
 * its file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_TRUSS_H_
#define GRAPHLILY_HIP_TRUSS_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K-TRUSS DECOMPOSITION over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_truss.hip), on a square
 * whole-matrix plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is symmetric
 * (io.symmetrize_simple prepares it).  An ENTRY is a stored (v, u); entry j is word j of the plan's row copy, in the caller's
 * order.  An EDGE is the pair of entries (v, u) and (u, v), u != v.  With nnz entries:
 *   d_truss[j]   = the largest k such that the edge of entry j lies in a subgraph in which every edge is in at least k - 2
 *                  triangles of that subgraph; an edge in no triangle has 2; both entries of an edge carry the same value; an
 *                  entry (v, v) gets 0                                                                      (nnz words)
 *   d_support[j] = |N(v) & N(u)|, the triangles through the edge; 0 for an entry (v, v)                    (nnz words, may be NULL)
 *   h_stats      = {max_truss, levels, sub_rounds, launches enqueued, edges, triangles}                    (6 HOST words, may be NULL)
 *                  levels = distinct truss values; sub_rounds = the slices the queue was cut into, a property of the graph;
 *                  triangles = the sum of the supports over the edges / 3
 * Both arrays are fully written by the call itself; the result is unique: two calls give the same bits.
 * The edges are numbered once per plan (entries above the diagonal in row order; the mirror entry finds its partner by binary
 * search).  A support pass intersects the two rows of every edge.  The peel then works level by level, l = truss - 2: a
 * device-resident queue receives every edge whose word has come down to l, one launch per sub-round takes a slice of the queue
 * and takes one triangle from the two other edges of every triangle that it destroys, each launch gated by a control record on
 * the device, so the result does not depend on how many launches are enqueued at a time.
 * GL_ERR_UNSUPPORTED for a plan without the row copy, with num_rows != num_cols, for a row shard, for rows that are not strictly
 * ascending or hold a column >= num_cols (a zero-valued entry is stored as 0xffffffff), and for a pattern that is not symmetric.
 * A NULL plan or d_truss, or d_support == d_truss, is GL_ERR_INVALID_ARG.  A plan without entries (planned in the general layout
 * whatever its flags) writes nothing and h_stats is zero.
 * THE CALL SYNCHRONISES: the host enqueues a fixed batch of gated launches, copies the control record to page-locked memory and
 * waits, once per batch, until the record says done (at most 2 edges + 1 steps exist; GL_ERR_HIP with the record's contents
 * should the cap ever be hit).  A plan's first call also establishes the verdicts that the k-core and colouring passes cache,
 * numbers the edges (one more wait) and allocates 256 + 4 (num_rows + 1 + nnz + 5 (nnz / 2)) bytes of scratch, which
 * gl_spmv_plan_destroy frees. */
int gl_truss(gl_spmv_plan plan, uint32_t *d_truss, uint32_t *d_support /* may be NULL */, uint64_t *h_stats /* may be NULL, 6 words */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_TRUSS_H_ */
