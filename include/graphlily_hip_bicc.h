/*
 * graphlily_hip_bicc.h -- the biconnected-components extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry point of gl_bicc.hip and nothing else, and capi.EXT_HEADERS maps its
 * file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_BICC_H_
#define GRAPHLILY_HIP_BICC_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* BICONNECTED COMPONENTS over the plain CSR copy a GL_PLAN_BOOLEAN plan keeps (gl_bicc.hip).  The plan is read as
 * an undirected simple graph, exactly as gl_truss reads it: a square whole-matrix plan whose rows are strictly ascending sets of
 * columns below num_cols and whose pattern is symmetric (io.symmetrize_simple prepares the matrix).  Entry j is word j of the row
 * copy, an EDGE is the pair of entries (v, u) and (u, v).  With n = num_rows vertices and nnz entries:
 *   d_block[j]           = the SMALLEST ENTRY NUMBER of the block (biconnected component: a class of "two edges lie on a common
 *                          simple cycle", a bridge being a block of its own) that holds entry j's edge; both entries of an edge
 *                          agree; an entry (v, v), should the contract ever admit one, gets 0xffffffff            (nnz words)
 *   d_vertex_blocks[v]   = the number of blocks v belongs to: 0 for an isolated vertex, >= 2 for an ARTICULATION POINT
 *                                                                                                      (n words, may be NULL)
 *   d_edge_component[v]  = the smallest vertex of v's 2-EDGE-CONNECTED component: gl_cc_labels' labelling of the graph without
 *                          its bridges (an edge whose block has no other edge)                          (n words, may be NULL)
 *   d_tree               = a diagnostic copy of the intermediate arrays {level, parent, pre, nd, low, high}, n words each: the
 *                          tests name the phase that went wrong with it                               (6 n words, may be NULL)
 *   h_stats              = {blocks, articulation points, bridges, depth, launches enqueued, trees}; depth is the largest level
 *                          of the forest                                                           (6 HOST words, may be NULL)
 * All of them are unique -- functions of the graph, whatever the schedule -- and nothing is floating point.
 * THE METHOD is Tarjan and Vishkin's over a DETERMINISTIC BFS forest.  The rule of every array:
 *   roots     r is a root iff gl_cc_labels would label it with itself (isolated vertices included)
 *   level     the distance from the root of the vertex's component; found by a multi-source search from all roots, one gated
 *             launch per level, a vertex claimed by a compare-and-swap on its level word
 *   parent    the smallest neighbour one level up; parent[root] = root
 *   nd        the size of the subtree below (and with) the vertex
 *   pre       preorder, local to each tree: pre[root] = 0, and the children c of v IN ASCENDING VERTEX ORDER get pre[v] + 1 + the
 *             nd of the earlier children
 *   low/high  the min / max over the subtree of v of pre[x] and of pre[u] for the NON-TREE neighbours u of x (an entry is
 *             non-tree when neither end is the other's parent)
 *   blocks    a tree edge is named by its child.  The edges named v and w are united when w is a child of v, v is no root and
 *             low[w] < pre[v] || high[w] >= pre[v] + nd[v]; and when (v, w) is a non-tree entry with pre[v] + nd[v] <= pre[w].
 *             The block of an entry is that of the child end of a tree edge, of the end with the larger pre otherwise.
 *   bridges   a tree edge to child c with low[c] >= pre[c] && high[c] < pre[c] + nd[c]
 *   vertex_blocks[v] = (v is no root ? 1 : 0) + the blocks whose top -- the parent of the block's shallowest child -- is v
 * GL_ERR_UNSUPPORTED, in gl_truss' order and wording: a plan without the row copy, with num_rows != num_cols, a row shard, rows
 * that are not strictly ascending or hold a zero-valued entry or a column >= num_cols, a pattern that is not symmetric (checked
 * on the device on first use and cached in the plan).  GL_ERR_INVALID_ARG for a NULL plan or d_block and for outputs that overlap.
 * A plan without entries writes zeros to d_vertex_blocks, v to d_edge_component[v] and the trivial forest (level 0, parent v, pre
 * 0, nd 1, low 0, high 0) to d_tree, and reports {0, 0, 0, 0, launches, n}.
 * THE CALL SYNCHRONISES, as gl_truss does: the host enqueues a fixed batch of (level step, turn) launch pairs, every launch gated
 * by a control record on the device, copies the record to page-locked memory and waits, once per batch, until the record says that
 * every vertex has its level.  It then enqueues 3 depth + a dozen launches blindly -- one per level for nd, pre and low / high,
 * which read their slice of the level-ordered queue on the device -- and waits once more.  A search that is not done after n steps
 * ends with GL_ERR_HIP ("internal error") instead of hanging.  A PATH of n vertices is the worst case: 5 n launches.
 * The first call also establishes the verdicts named above and allocates 256 + 4 (16 num_rows + 2) bytes of scratch -- the control
 * record, a 64-bit word per vertex for the blocks' tops, the six arrays of d_tree, the queue, the roots, two union-find arrays, the
 * blocks' first entries, the bridge flags, the top counts and num_rows + 2 level offsets -- which gl_spmv_plan_destroy frees. */
int gl_bicc(gl_spmv_plan plan, uint32_t *d_block /* nnz */, uint32_t *d_vertex_blocks /* num_rows, may be NULL */, uint32_t *d_edge_component /* num_rows, may be NULL */, uint32_t *d_tree /* 6 num_rows, may be NULL */, uint64_t *h_stats /* 6 HOST words, may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_BICC_H_ */
