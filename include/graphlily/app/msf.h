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

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <utility>
#include <vector>

namespace graphlily {
namespace app {

class MinimumSpanningForest : public app::ModuleCollection {
private:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *SpMV_;
    uint32_t matrix_num_rows_ = 0, matrix_num_cols_ = 0;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    graphlily::SemiringType semiring_ = graphlily::LogicalSemiring;
    uint32_t n_real_ = 0;
    bool sent_ = false;
    CSRMatrix<float> graph_;
    DeviceBuffer weight_;
    std::vector<uint32_t> degrees_, labels_;
    std::vector<std::pair<uint32_t, uint32_t>> edges_;
    std::vector<float> weights_;
    double total_weight_ = 0.0;
    uint64_t num_edges_ = 0, num_components_ = 0, rounds_ = 0, launches_ = 0;

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_forest_vec_t;

    MinimumSpanningForest(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
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
    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric matrix, weights in adj_data: what results align with

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, bool weighted = true) {
        CSRMatrix<float> csr_matrix = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        n_real_ = csr_matrix.num_rows;
        graphlily::io::util_round_csr_matrix_dim(csr_matrix, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        graph_ = graphlily::io::util_symmetrize_weighted(csr_matrix, degrees_, weighted);      // after padding
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

    // in_forest[j] = 1 if the edge of entry j of graph() is in the forest; leaves edges(), weights(), total_weight(), num_edges(),
    // num_components() (over the real vertices: padding vertices are singletons), rounds(), launches() and, with want_labels,
    // labels().  The call waits for the device.
    aligned_forest_vec_t run(bool want_labels = false) {
        if (!sent_) {
            printf("MinimumSpanningForest::run(): send_matrix_host_to_device first\n");
            exit(EXIT_FAILURE);
        }
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
        edges_.clear();
        weights_.clear();
        total_weight_ = 0.0;
        for (size_t v = 0; v < n; v++)
            for (uint32_t j = graph_.adj_indptr[v]; j < graph_.adj_indptr[v + 1]; j++)
                if (words[j] && graph_.adj_indices[j] > v) {               // once per edge, in entry order: (lo, hi) ascending
                    edges_.push_back(std::make_pair((uint32_t)v, graph_.adj_indices[j]));
                    weights_.push_back(graph_.adj_data[j]);
                    total_weight_ += (double)graph_.adj_data[j];
                }
        return words;
    }
    uint64_t num_edges() const { return num_edges_; }
    uint64_t num_components() const { return num_components_; }
    uint64_t rounds() const { return rounds_; }                                    // Boruvka rounds in which a component chose an edge
    uint64_t launches() const { return launches_; }
    double total_weight() const { return total_weight_; }                          // the f64 sum of weights() in entry order
    const std::vector<std::pair<uint32_t, uint32_t>> &edges() const { return edges_; }   // (lo, hi), ascending
    const std::vector<float> &weights() const { return weights_; }
    const std::vector<uint32_t> &labels() const { return labels_; }               // empty unless run(true)
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_MSF_H_
