// graphlily/app/msf.h -- minimum spanning forest over the MI355X backend (an extension: the reference has no such driver), with
// the conventions of the drivers next to it (graphlily/app/truss.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_msf walks
// (include/graphlily_hip_msf.h).  The matrix is read as an undirected weighted graph and stored in both
// directions by the host (graphlily::io::util_symmetrize_weighted: the diagonal dropped, every other stored entry an edge, the
// smallest value of an edge stored more than once, -0.0 as +0.0, NaN refused; weighted = false: zero values are no edges and
// every weight is 1); that matrix is kept as graph(), with the weights in adj_data, and an all-ones copy of it is planned.  Every
// result has one word per ENTRY of graph(), aligned with graph().adj_indices: both entries of an edge carry the same value.
//   edges are ordered by (key(w), lo, hi), a strict total order: the forest is unique, Kruskal's in that order
// Row shards are not supported: the kernel reads the component of every column of a row and the rows of both ends of an edge.
#ifndef GRAPHLILY_HIP_APP_MSF_H_
#define GRAPHLILY_HIP_APP_MSF_H_

#include "graphlily/app/pattern_app.h"

#include <vector>

namespace graphlily {
namespace app {

class MinimumSpanningForest : public app::WeightedPatternApp {
private:
    bool weighted_ = true;
    std::vector<uint32_t> labels_;
    uint64_t num_edges_ = 0, num_components_ = 0, rounds_ = 0, launches_ = 0;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        graph_ = graphlily::io::util_symmetrize_weighted(padded, degrees_, weighted_);
        return ones_of_graph();
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_forest_vec_t;

    MinimumSpanningForest(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : WeightedPatternApp("MinimumSpanningForest", num_channels, spmv_out_buf_len, vec_buf_len) {}

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, bool weighted = true) {
        weighted_ = weighted;
        WeightedPatternApp::load_and_format_matrix(csr_float_npz_path, skip_empty_rows);
    }

    // in_forest[j] = 1 if the edge of entry j of graph() is in the forest; leaves edges(), weights(), total_weight(), num_edges(),
    // num_components() (over the real vertices: padding vertices are singletons), rounds(), launches() and, with want_labels,
    // labels().  The call waits for the device.
    aligned_forest_vec_t run(bool want_labels = false) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, nnz = graph_.adj_indices.size(), room = nnz ? nnz : 1;
        DeviceBuffer out(sizeof(uint32_t) * (room + (want_labels ? n : 0)));      // the forest words, then the labels
        uint64_t stats[4] = {0, 0, 0, 0};
        SpMV_->msf(weight_, out, want_labels && n ? (uint32_t *)out.ptr() + room : nullptr, stats);
        aligned_forest_vec_t words(room + (want_labels ? n : 0));
        out.download(words.data(), sizeof(uint32_t) * words.size());
        labels_.assign(words.begin() + room, words.end());
        words.resize(nnz);
        num_edges_ = stats[0];
        num_components_ = stats[1] - (n - n_real_);
        rounds_ = stats[2];
        launches_ = stats[3];
        collect_edges([&](size_t, uint32_t j) { return words[j] != 0; });
        return words;
    }
    uint64_t num_edges() const { return num_edges_; }
    uint64_t num_components() const { return num_components_; }
    uint64_t rounds() const { return rounds_; }                                    // Boruvka rounds in which a component chose an edge
    uint64_t launches() const { return launches_; }
    const std::vector<uint32_t> &labels() const { return labels_; }               // empty unless run(true)
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_MSF_H_
