/*
 * graphlily_hip_contract.h -- the graph contraction extension to the C ABI of libgraphlily_hip.so (graphlily_hip.h).
 *
 * ONE HEADER PER EXTENSION: this header declares the entry points of gl_contract.hip and nothing else, and capi.EXT_HEADERS maps
 * its file name to the names it declares; the suite and the build check that entry against this header and against the library.
 * The conventions are those of graphlily_hip.h: a gl_status is returned, gl_last_error gives the message, `d_` parameters are
 * device pointers, `h_` parameters host pointers, work goes to the library's current stream.
 */
#ifndef GRAPHLILY_HIP_CONTRACT_H_
#define GRAPHLILY_HIP_CONTRACT_H_

#include "graphlily_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Graph contraction: the quotient C = S^T A S of the graph in the plan's plain CSR row copy (a GL_PLAN_BOOLEAN plan) by a
 * labelling of its vertices, in exact 32-bit integer weights (gl_contract.hip).  The plan is square, whole, its
 * rows strictly ascending sets of columns; symmetry is NOT required: a directed pattern contracts too.  Only the first
 * num_vertices <= num_rows vertices are labelled; the rows at and behind num_vertices (a level's padding vertices) must be
 * empty, and a column at or behind num_vertices is no entry.  d_label[v] < num_vertices is any vertex number (gl_louvain_move's,
 * gl_cc_labels' and gl_scc's labels are).
 *
 * THE DEFINITION is io.aggregate_communities', made direction-aware.  The groups are numbered 0 .. k - 1 in ascending order of
 * their labels and part[v] is the number of v's group.  C has an entry (a, b), a != b, iff some stored entry (v, u) has
 * part[v] = a and part[u] = b; its weight is the sum of those entries' weights.  C has no diagonal, the columns of every row
 * ascend, c_indptr[0] = 0.  tot[a] is the sum of k[v] over the members of a; a k[v] that is not given is the sum of the weights
 * of row v's entries off the diagonal.  Sums are formed in 64 bits; a sum above 0xffffffff is stored as 0xffffffff and counted.
 *
 *   gl_contract_symbolic  writes the num_vertices words of d_part and the k + 1 words of d_c_indptr and SYNCHRONISES.
 *   gl_contract_numeric   takes the d_part, k and d_c_indptr of the LAST symbolic call on this plan (whose grouping the plan
 *                         keeps) and writes the nnz(C) words of d_c_indices and d_c_weight and the k words of d_tot.  d_weight[j]
 *                         is the weight of entry j of the row copy.  IT ONLY ENQUEUES, unless h_stats is given.
 * h_stats (6 HOST words) = {k, nnz(C), bound, groups that took the workgroup path, groups that took the slab path, saturated
 * sums}; bound = the sum of the row lengths; symbolic reports no saturated sums.  Nothing behind word k + 1 of d_c_indptr, word
 * nnz(C) of d_c_indices / d_c_weight, word k of d_tot or word num_vertices of d_part is written.  A plan without entries gives
 * part, tot and k + 1 zeros.
 *
 * HOW: a presence bitmap over the labels and a popcount prefix rank them; a counting sort groups the vertices by part; then one
 * agent per group walks the rows of ALL its members as one concatenated entry stream -- per window of 64 members a prefix scan of
 * the row lengths goes to LDS and the lanes take consecutive positions of the stream, finding their member by a search in the
 * 64 offsets -- and inserts part[column] into a table of (key, 64-bit sum) slots claimed by compare-and-swap on 0xffffffff,
 * linear probing.  Three paths, chosen per group by a count (symbolic: the group's entries, an upper bound; numeric: |C(a)|): a
 * wavefront with GRAPHLILY_DEBUG contract_wave_slots (512) slots in LDS; a workgroup with contract_lds_slots (8192) slots in
 * dynamic LDS; a dense slab over the k columns (a bitmap and a 64-bit word per column) in one of a fixed number of global slabs.
 * contract_wave=0 / contract_lds=0 close the first / the first two paths; contract_grid = workgroups per compute unit of the
 * wavefront path.  The hash paths compact and sort their slots in LDS (counting up to 64, bitonic above), the slab emits from
 * its bitmap.  No floating point anywhere.
 *
 * GL_ERR_INVALID_ARG: a NULL plan, d_label, d_part, d_c_indptr, d_c_indices or symbolic h_stats; num_vertices > num_rows; a
 * label >= num_vertices; a numeric call whose num_vertices or k is not the last symbolic call's.
 * GL_ERR_UNSUPPORTED: what gl_tc_count refuses of a plan (no row copy, num_rows != num_cols, a row shard, entries that do not fit
 * 32-bit offsets, rows that are no strictly ascending sets); a non-empty row at or behind num_vertices; nnz(C) >= 2^32. */
int gl_contract_symbolic(gl_spmv_plan plan, uint32_t num_vertices, const uint32_t *d_label, uint32_t *d_part /* num_vertices words, out */, uint32_t *d_c_indptr /* room for num_vertices + 1 words; k + 1 are written */, uint64_t *h_stats /* 6 HOST words, required */);
int gl_contract_numeric(gl_spmv_plan plan, uint32_t num_vertices, const uint32_t *d_part, uint32_t k, const uint32_t *d_weight /* may be NULL: every entry 1 */, const uint32_t *d_vertex_weight /* may be NULL: the sum of the row's entry weights */, const uint32_t *d_c_indptr, uint32_t *d_c_indices, uint32_t *d_c_weight /* may be NULL: the pattern only */, uint32_t *d_tot /* k words, may be NULL */, uint64_t *h_stats /* 6 HOST words, may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* GRAPHLILY_HIP_CONTRACT_H_ */
