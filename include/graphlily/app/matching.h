// graphlily/app/matching.h -- greedy weighted matching over the MI355X backend (an extension: the reference has no such driver),
// with the conventions of the drivers next to it (graphlily/app/msf.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_match walks
// (include/graphlily_hip_match.h).  The matrix is read as an undirected weighted graph and stored in both
// directions by the host (graphlily::io::util_symmetrize_weighted with keep_largest: the diagonal dropped, every other stored
// entry an edge, the LARGEST value of an edge stored more than once, -0.0 as +0.0, NaN refused; weighted = false: zero values are
// no edges and every weight is 1; drop_nonpositive: the edges of weight <= 0 are removed); that matrix is kept as graph(), with
// the weights in adj_data, and an all-ones copy of it is planned.
//   edges are ordered by (~key(w), lo, hi) -- heaviest first, then the smallest (lo, hi) --, a strict total order: the result is
//   unique, the matching that takes the edges greedily in that order
// Row shards are not supported: the kernel reads the mate of every column of a row and the rows of both ends of a matched edge.
#ifndef GRAPHLILY_HIP_APP_MATCHING_H_
#define GRAPHLILY_HIP_APP_MATCHING_H_

#include "graphlily/app/pattern_app.h"

#include <vector>

namespace graphlily {
namespace app {

class Matching : public app::WeightedPatternApp {
private:
    bool weighted_ = true, drop_nonpositive_ = false;
    std::vector<uint32_t> mate_;
    uint64_t num_matched_ = 0, rounds_ = 0, scans_ = 0, launches_ = 0;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        graph_ = graphlily::io::util_symmetrize_weighted(padded, degrees_, weighted_, true);
        if (drop_nonpositive_) {
            CSRMatrix<float> kept;
            kept.num_rows = graph_.num_rows;
            kept.num_cols = graph_.num_cols;
            kept.adj_indptr.assign(graph_.num_rows + 1, 0);
            for (uint32_t v = 0; v < graph_.num_rows; v++) {
                for (uint32_t j = graph_.adj_indptr[v]; j < graph_.adj_indptr[v + 1]; j++)
                    if (graph_.adj_data[j] > 0.0f) {
                        kept.adj_indices.push_back(graph_.adj_indices[j]);
                        kept.adj_data.push_back(graph_.adj_data[j]);
                    }
                kept.adj_indptr[v + 1] = (uint32_t)kept.adj_indices.size();
                degrees_[v] = kept.adj_indptr[v + 1] - kept.adj_indptr[v];
            }
            graph_ = kept;
        }
        return ones_of_graph();
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_mate_vec_t;
    static const uint32_t kFree = 0xffffffffu;                       // mate()[v] of a vertex that stays free

    Matching(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : WeightedPatternApp("Matching", num_channels, spmv_out_buf_len, vec_buf_len) {}

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, bool weighted = true, bool drop_nonpositive = false) {
        weighted_ = weighted;
        drop_nonpositive_ = drop_nonpositive;
        WeightedPatternApp::load_and_format_matrix(csr_float_npz_path, skip_empty_rows);
    }

    // mate[v] = the vertex v is matched to, kFree for a free vertex; leaves edges(), weights(), total_weight(), num_matched(),
    // rounds(), scans() and launches().  The call waits for the device.
    aligned_mate_vec_t run() {
        require_sent("run()");
        const size_t n = matrix_num_rows_;
        DeviceBuffer out(sizeof(uint32_t) * (n ? n : 1));
        uint64_t stats[4] = {0, 0, 0, 0};
        SpMV_->match(weight_, out, stats);
        aligned_mate_vec_t mate(n ? n : 1);
        out.download(mate.data(), sizeof(uint32_t) * mate.size());
        mate.resize(n);
        mate_.assign(mate.begin(), mate.end());
        num_matched_ = stats[0];
        rounds_ = stats[1];
        scans_ = stats[2];
        launches_ = stats[3];
        collect_edges([&](size_t v, uint32_t j) { return mate[v] == graph_.adj_indices[j]; });
        return mate;
    }
    const std::vector<uint32_t> &mate() const { return mate_; }                   // the last run()'s result
    uint64_t num_matched() const { return num_matched_; }                         // matched edges
    uint64_t rounds() const { return rounds_; }                                    // rounds in which a vertex pointed or finished
    uint64_t scans() const { return scans_; }                                      // row scans of all rounds
    uint64_t launches() const { return launches_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_MATCHING_H_
