// graphlily/app/truss.h -- k-truss decomposition over the MI355X backend (an extension: the reference has no such driver), with
// the conventions of the drivers next to it (graphlily/app/kcore.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_truss walks
// (include/graphlily_hip_truss.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and stored in both directions by the host
// (graphlily::io::util_symmetrize_simple); that matrix is kept as graph(), and every result has one word per ENTRY of it, aligned
// with graph().adj_indices: both entries of an edge carry the same value.
//   truss[j] = the largest k such that the edge of entry j lies in a subgraph in which every edge is in >= k - 2 triangles
// Row shards are not supported: the kernel reads row u for every column u of a row.
#ifndef GRAPHLILY_HIP_APP_TRUSS_H_
#define GRAPHLILY_HIP_APP_TRUSS_H_

#include "graphlily/app/pattern_app.h"

#include <vector>

namespace graphlily {
namespace app {

class KTruss : public app::PatternApp {
private:
    CSRMatrix<float> graph_;
    std::vector<uint32_t> support_, vertex_truss_;
    std::vector<uint64_t> truss_sizes_;
    uint64_t max_truss_ = 0, levels_ = 0, sub_rounds_ = 0, launches_ = 0, num_edges_ = 0, num_triangles_ = 0;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        graph_ = graphlily::io::util_symmetrize_simple(padded, degrees_);
        return graph_;
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_truss_vec_t;

    KTruss(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("KTruss", num_channels, spmv_out_buf_len, vec_buf_len) {}

    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric simple matrix the results are aligned with

    // the truss number of every entry's edge; leaves max_truss(), levels(), sub_rounds(), launches(), num_edges(),
    // num_triangles(), truss_sizes(), vertex_truss() and, with want_support, support().  The call waits for the device.
    aligned_truss_vec_t run(bool want_support = false) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, nnz = graph_.adj_indices.size(), words = want_support ? 2 * nnz : nnz;
        DeviceBuffer out(sizeof(uint32_t) * (words ? words : 1));    // the truss numbers, then the supports
        uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
        SpMV_->truss(out, want_support && nnz ? (uint32_t *)out.ptr() + nnz : nullptr, stats);
        aligned_truss_vec_t truss(words);
        if (words) out.download(truss.data(), sizeof(uint32_t) * words);
        support_.assign(truss.begin() + nnz, truss.end());
        truss.resize(nnz);
        max_truss_ = stats[0];
        levels_ = stats[1];
        sub_rounds_ = stats[2];
        launches_ = stats[3];
        num_edges_ = stats[4];
        num_triangles_ = stats[5];
        std::vector<uint64_t> count((size_t)max_truss_ + 2, 0);
        vertex_truss_.assign(n, 0);
        for (size_t v = 0; v < n; v++) {
            for (uint32_t j = graph_.adj_indptr[v]; j < graph_.adj_indptr[v + 1]; j++) {
                if (truss[j] > vertex_truss_[v]) vertex_truss_[v] = truss[j];
                if (graph_.adj_indices[j] > v) count[truss[j] <= max_truss_ ? truss[j] : max_truss_ + 1]++;
            }
        }
        truss_sizes_.assign((size_t)max_truss_ + 1, 0);
        uint64_t above = count[(size_t)max_truss_ + 1];
        for (size_t k = (size_t)max_truss_ + 1; k-- > 0;) truss_sizes_[k] = above += count[k];
        return truss;
    }
    uint64_t max_truss() const { return max_truss_; }                            // 0 for a graph without edges
    uint64_t levels() const { return levels_; }
    uint64_t sub_rounds() const { return sub_rounds_; }
    uint64_t launches() const { return launches_; }
    uint64_t num_edges() const { return num_edges_; }
    uint64_t num_triangles() const { return num_triangles_; }
    const std::vector<uint32_t> &support() const { return support_; }            // empty unless run(true)
    const std::vector<uint32_t> &vertex_truss() const { return vertex_truss_; }  // the largest truss among a vertex's edges
    const std::vector<uint64_t> &truss_sizes() const { return truss_sizes_; }    // [k] = edges with truss >= k
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_TRUSS_H_
