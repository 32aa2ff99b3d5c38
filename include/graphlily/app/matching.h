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

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <utility>
#include <vector>

namespace graphlily {
namespace app {

class Matching : public app::ModuleCollection {
private:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *SpMV_;
    uint32_t matrix_num_rows_ = 0, matrix_num_cols_ = 0;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    graphlily::SemiringType semiring_ = graphlily::LogicalSemiring;
    uint32_t n_real_ = 0;
    bool sent_ = false;
    CSRMatrix<float> graph_;
    DeviceBuffer weight_;
    std::vector<uint32_t> degrees_;
    std::vector<std::pair<uint32_t, uint32_t>> edges_;
    std::vector<float> weights_;
    double total_weight_ = 0.0;
    uint64_t num_matched_ = 0, rounds_ = 0, scans_ = 0, launches_ = 0;

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_mate_vec_t;
    static const uint32_t kFree = 0xffffffffu;                       // mate()[v] of a vertex that stays free

    Matching(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : num_channels_(num_channels), spmv_out_buf_len_(spmv_out_buf_len), vec_buf_len_(vec_buf_len) {
        SpMV_ = new graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t>(num_channels_, spmv_out_buf_len_, vec_buf_len_);
        SpMV_->set_semiring(semiring_);
        SpMV_->set_mask_type(graphlily::kNoMask);
        add_module(SpMV_);
    }

    uint32_t get_nnz() { return SpMV_->get_nnz(); }                 // entries of the symmetric matrix: twice the undirected edges
    uint32_t num_vertices() const { return matrix_num_rows_; }      // the padded matrix's
    uint32_t num_real_vertices() const { return n_real_; }
    const std::vector<uint32_t> &degrees() const { return degrees_; }
    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric matrix, weights in adj_data

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, bool weighted = true, bool drop_nonpositive = false) {
        CSRMatrix<float> csr_matrix = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        n_real_ = csr_matrix.num_rows;
        graphlily::io::util_round_csr_matrix_dim(csr_matrix, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        graph_ = graphlily::io::util_symmetrize_weighted(csr_matrix, degrees_, weighted, true);      // after padding
        if (drop_nonpositive) {
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
        CSRMatrix<float> ones = graph_;                                    // a zero value would be stored as no entry: plan ones
        ones.adj_data.assign(ones.adj_indices.size(), 1.0f);
        SpMV_->load_and_format_matrix(ones, skip_empty_rows);
        matrix_num_rows_ = SpMV_->get_num_rows();
        matrix_num_cols_ = SpMV_->get_num_cols();
        assert(matrix_num_rows_ == matrix_num_cols_);
        sent_ = false;
    }

    void send_matrix_host_to_device() {
        SpMV_->send_matrix_host_to_device();
        const size_t nnz = graph_.adj_data.size();
        weight_ = DeviceBuffer(sizeof(float) * (nnz ? nnz : 1));
        if (nnz) weight_.upload(graph_.adj_data.data(), sizeof(float) * nnz);
        sent_ = true;
    }

    // mate[v] = the vertex v is matched to, kFree for a free vertex; leaves edges(), weights(), total_weight(), num_matched(),
    // rounds(), scans() and launches().  The call waits for the device.
    aligned_mate_vec_t run() {
        if (!sent_) {
            printf("Matching::run(): send_matrix_host_to_device first\n");
            exit(EXIT_FAILURE);
        }
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
        edges_.clear();
        weights_.clear();
        total_weight_ = 0.0;
        for (size_t v = 0; v < n; v++)
            for (uint32_t j = graph_.adj_indptr[v]; j < graph_.adj_indptr[v + 1]; j++)
                if (graph_.adj_indices[j] > v && mate[v] == graph_.adj_indices[j]) {   // once per edge, in entry order: (lo, hi) ascending
                    edges_.push_back(std::make_pair((uint32_t)v, graph_.adj_indices[j]));
                    weights_.push_back(graph_.adj_data[j]);
                    total_weight_ += (double)graph_.adj_data[j];
                }
        return mate;
    }
    const std::vector<uint32_t> &mate() const { return mate_; }                   // the last run()'s result
    uint64_t num_matched() const { return num_matched_; }                         // matched edges
    uint64_t rounds() const { return rounds_; }                                    // rounds in which a vertex pointed or finished
    uint64_t scans() const { return scans_; }                                      // row scans of all rounds
    uint64_t launches() const { return launches_; }
    double total_weight() const { return total_weight_; }                          // the f64 sum of weights() in entry order
    const std::vector<std::pair<uint32_t, uint32_t>> &edges() const { return edges_; }   // (lo, hi), ascending
    const std::vector<float> &weights() const { return weights_; }

private:
    std::vector<uint32_t> mate_;
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_MATCHING_H_
