// graphlily/app/quotient.h -- the quotient of a graph by a labelling of its vertices over the MI355X backend (an extension: the
// reference has no such driver; the C++ counterpart of QuotientGraph in graphlily_amd/app.py), with the conventions of the drivers
// next to it (graphlily/app/kcore.h): print and exit on error, device-resident buffers.  One SpMVModule with the (||,&&) semiring,
// so that the plan is the boolean layout, whose plain row copy gl_contract walks (include/graphlily_hip_contract.h, DESIGN.md
// 4.30).  The matrix is read as a simple graph -- zero values, the diagonal and duplicates dropped --, undirected and stored in
// both directions (graphlily::io::util_symmetrize_simple) or directed (graphlily::io::util_simple_pattern: an entry (v, u) for an
// edge u -> v).  Vertices with one label become one vertex, parallel edges are summed in exact 32-bit integers, what falls inside
// a group goes to the group's weight alone.
// Row shards are not supported: a group's members lie anywhere in the matrix, so every rank would need every row.
#ifndef GRAPHLILY_HIP_APP_QUOTIENT_H_
#define GRAPHLILY_HIP_APP_QUOTIENT_H_

#include "graphlily/app/pattern_app.h"
#include "graphlily_hip_contract.h"

#include <vector>

namespace graphlily {
namespace app {

class QuotientGraph : public app::PatternApp {
private:
    CSRMatrix<float> graph_, quotient_;
    std::vector<uint32_t> weights_, tot_, community_of_;
    int directed_asked_ = -1;
    bool directed_ = false;
    uint32_t num_groups_ = 0, paths_[3] = {0, 0, 0};
    uint64_t inside_weight_ = 0;

    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        CSRMatrix<float> out;
        const bool symmetric = graphlily::io::util_simple_pattern(padded, graph_, out);
        directed_ = directed_asked_ < 0 ? !symmetric : directed_asked_ != 0;
        if (!directed_) graph_ = graphlily::io::util_symmetrize_simple(padded, degrees_);
        return graph_;
    }

public:
    QuotientGraph(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("QuotientGraph", num_channels, spmv_out_buf_len, vec_buf_len) {}

    // directed < 0: undirected iff the pattern is symmetric; 0 takes every edge in both directions; > 0 keeps the direction
    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, int directed = -1) {
        directed_asked_ = directed;
        PatternApp::load_and_format_matrix(csr_float_npz_path, skip_empty_rows);
    }

    // the quotient of graph() by `labels` (one vertex number per vertex, num_real_vertices() or num_vertices() of them), under
    // the entry weights `weights` (aligned with graph().adj_indices; empty: all 1) and the vertex weights `vertex_weights` (one per
    // label; empty: the sums of the entries' weights): the groups are numbered in ascending order of their labels.  Leaves
    // quotient(), weights(), tot(), community_of(), num_groups(), inside_weight() and paths().  A summed weight that does not fit
    // 32 bits is an error.  The call waits for the device.
    const CSRMatrix<float> &run(const std::vector<uint32_t> &labels, const std::vector<uint32_t> &weights = std::vector<uint32_t>(),
                                const std::vector<uint32_t> &vertex_weights = std::vector<uint32_t>()) {
        require_sent("run()");
        const size_t nv = labels.size(), nnz = graph_.adj_indices.size();
        if ((nv != n_real_ && nv != matrix_num_rows_) || (!weights.empty() && weights.size() != nnz) || (!vertex_weights.empty() && vertex_weights.size() != nv)) {
            printf("QuotientGraph::run(): %zu labels, %zu weights, %zu vertex weights for %u (%u) vertices and %zu entries\n", nv, weights.size(),
                   vertex_weights.size(), n_real_, matrix_num_rows_, nnz);
            exit(EXIT_FAILURE);
        }
        const size_t nv1 = nv ? nv : 1;
        DeviceBuffer in(sizeof(uint32_t) * (4 * nv1 + 1 + (nnz ? nnz : 1)));     // the labels, k, part, the offsets of C, the entry weights
        uint32_t *d_label = (uint32_t *)in.ptr(), *d_k = d_label + nv1, *d_part = d_k + nv1, *d_indptr = d_part + nv1, *d_w = d_indptr + nv1 + 1;
        if (nv) gl_buf_h2d(d_label, labels.data(), sizeof(uint32_t) * nv);
        if (!vertex_weights.empty()) gl_buf_h2d(d_k, vertex_weights.data(), sizeof(uint32_t) * nv);
        if (!weights.empty()) gl_buf_h2d(d_w, weights.data(), sizeof(uint32_t) * nnz);
        uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
        GRAPHLILY_CHECK(gl_contract_symbolic(SpMV_->plan_handle(), (uint32_t)nv, d_label, d_part, d_indptr, stats));
        const size_t k = stats[0], cnz = stats[1];
        DeviceBuffer out(sizeof(uint32_t) * (2 * cnz + k + 1));                   // the columns, the weights, tot
        uint32_t *d_idx = (uint32_t *)out.ptr(), *d_cw = d_idx + cnz, *d_tot = d_cw + cnz;
        GRAPHLILY_CHECK(gl_contract_numeric(SpMV_->plan_handle(), (uint32_t)nv, d_part, (uint32_t)k, weights.empty() ? nullptr : d_w,
                                            vertex_weights.empty() ? nullptr : d_k, d_indptr, d_idx, d_cw, d_tot, stats));
        if (stats[5]) {
            printf("QuotientGraph::run(): %llu summed weights do not fit 32 bits\n", (unsigned long long)stats[5]);
            exit(EXIT_FAILURE);
        }
        quotient_ = CSRMatrix<float>();
        quotient_.num_rows = quotient_.num_cols = (uint32_t)k;
        quotient_.adj_indptr.assign(k + 1, 0);
        quotient_.adj_indices.assign(cnz, 0);
        quotient_.adj_data.assign(cnz, 1.0f);
        weights_.assign(cnz, 0);
        tot_.assign(k, 0);
        community_of_.assign(nv, 0);
        gl_buf_d2h(quotient_.adj_indptr.data(), d_indptr, sizeof(uint32_t) * (k + 1));
        if (cnz) gl_buf_d2h(quotient_.adj_indices.data(), d_idx, sizeof(uint32_t) * cnz);
        if (cnz) gl_buf_d2h(weights_.data(), d_cw, sizeof(uint32_t) * cnz);
        if (k) gl_buf_d2h(tot_.data(), d_tot, sizeof(uint32_t) * k);
        if (nv) gl_buf_d2h(community_of_.data(), d_part, sizeof(uint32_t) * nv);
        num_groups_ = (uint32_t)k;
        uint64_t total = weights.empty() ? nnz : 0, outside = 0;
        for (uint32_t w : weights) total += w;
        for (uint32_t w : weights_) outside += w;
        inside_weight_ = total - outside;
        uint32_t rows_with = 0;
        for (size_t a = 0; a < k; a++) rows_with += quotient_.adj_indptr[a + 1] != quotient_.adj_indptr[a];
        paths_[1] = (uint32_t)stats[3];
        paths_[2] = (uint32_t)stats[4];
        paths_[0] = rows_with - paths_[1] - paths_[2];
        return quotient_;
    }

    bool directed() const { return directed_; }
    const CSRMatrix<float> &graph() const { return graph_; }                    // what the weights align with
    const CSRMatrix<float> &quotient() const { return quotient_; }
    const std::vector<uint32_t> &weights() const { return weights_; }           // aligned with quotient().adj_indices
    const std::vector<uint32_t> &tot() const { return tot_; }
    const std::vector<uint32_t> &community_of() const { return community_of_; }
    uint32_t num_groups() const { return num_groups_; }
    uint64_t inside_weight() const { return inside_weight_; }                   // the summed weight of the entries inside groups
    const uint32_t *paths() const { return paths_; }                            // groups on the wavefront, workgroup and slab path
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_QUOTIENT_H_
