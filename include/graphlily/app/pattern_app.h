// graphlily/app/pattern_app.h -- what the single-device drivers of the kernels that walk a boolean plan's plain row copy share
// (extensions: the reference has no such drivers; the C++ counterpart of _PatternApp in graphlily_amd/app.py): one SpMVModule
// with the (||,&&) semiring, so that the plan is the boolean layout, which keeps that copy; a matrix that prepare() turns into what
// the kernel accepts; print and exit on error, device-resident buffers.  Row shards are not supported: every driver's own header
// says why.  A new driver derives from PatternApp (WeightedPatternApp if its kernel takes a weight per entry), overrides prepare()
// and adds its run() and results.
#ifndef GRAPHLILY_HIP_APP_PATTERN_APP_H_
#define GRAPHLILY_HIP_APP_PATTERN_APP_H_

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <utility>
#include <vector>

namespace graphlily {
namespace app {

class PatternApp : public app::ModuleCollection {
protected:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *SpMV_;
    uint32_t matrix_num_rows_ = 0, matrix_num_cols_ = 0;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    graphlily::SemiringType semiring_ = graphlily::LogicalSemiring;
    uint32_t n_real_ = 0;
    bool sent_ = false;
    const char *name_;                      // the driver's class name, for its messages
    std::vector<uint32_t> degrees_;         // of the padded matrix's vertices in the graph prepare() made, if it counts them

    PatternApp(const char *name, uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : num_channels_(num_channels), spmv_out_buf_len_(spmv_out_buf_len), vec_buf_len_(vec_buf_len), name_(name) {
        SpMV_ = new graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t>(num_channels_, spmv_out_buf_len_, vec_buf_len_);
        SpMV_->set_semiring(semiring_);
        SpMV_->set_mask_type(graphlily::kNoMask);
        add_module(SpMV_);
    }

    // -> the matrix to plan, from the padded one (padding vertices have empty rows).  The default: every stored entry is an
    // edge, as in BFS
    virtual CSRMatrix<float> prepare(CSRMatrix<float> &padded) {
        for (auto &x : padded.adj_data) x = 1;
        return std::move(padded);
    }

    void require_sent(const char *what) {
        if (!sent_) {
            printf("%s::%s: send_matrix_host_to_device first\n", name_, what);
            exit(EXIT_FAILURE);
        }
    }

    // gl_kcore on the same plan -> a degeneracy ordering of the padded matrix's vertices (what the "smallest_last" colouring order
    // is made of) and, if asked for, the degeneracy.  The call waits for the device.
    std::vector<uint32_t> peel_order(uint32_t *degeneracy = nullptr) {
        const size_t n = matrix_num_rows_;
        DeviceBuffer peel(sizeof(uint32_t) * 2 * (n ? n : 1));      // the core numbers, then the order
        uint32_t stats[4] = {0, 0, 0, 0};
        SpMV_->kcore(peel, (uint32_t *)peel.ptr() + n, stats);
        std::vector<uint32_t> words(2 * n);
        peel.download(words.data(), sizeof(uint32_t) * 2 * n);
        if (degeneracy) *degeneracy = stats[0];
        return std::vector<uint32_t>(words.begin() + n, words.end());
    }

public:
    uint32_t get_nnz() { return SpMV_->get_nnz(); }                 // entries of the planned matrix
    uint32_t num_vertices() const { return matrix_num_rows_; }      // the padded matrix's
    uint32_t num_real_vertices() const { return n_real_; }
    const std::vector<uint32_t> &degrees() const { return degrees_; }

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows) {
        CSRMatrix<float> csr_matrix = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        n_real_ = csr_matrix.num_rows;
        graphlily::io::util_round_csr_matrix_dim(csr_matrix, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        SpMV_->load_and_format_matrix(prepare(csr_matrix), skip_empty_rows);      // (prepare() sees the matrix after padding)
        matrix_num_rows_ = SpMV_->get_num_rows();
        matrix_num_cols_ = SpMV_->get_num_cols();
        assert(matrix_num_rows_ == matrix_num_cols_);
        sent_ = false;
    }

    void send_matrix_host_to_device() {
        SpMV_->send_matrix_host_to_device();
        sent_ = true;
    }
};

// ... and of those whose kernels take a weight per entry: prepare() leaves the symmetric weighted matrix in graph_ and returns
// ones_of_graph(), because the row copy would store a zero value as no entry; the weights travel in a buffer of their own, aligned
// with graph().adj_indices.
class WeightedPatternApp : public PatternApp {
protected:
    CSRMatrix<float> graph_;
    DeviceBuffer weight_;
    std::vector<std::pair<uint32_t, uint32_t>> edges_;
    std::vector<float> weights_;
    double total_weight_ = 0.0;

    using PatternApp::PatternApp;

    CSRMatrix<float> ones_of_graph() const {
        CSRMatrix<float> ones = graph_;
        ones.adj_data.assign(ones.adj_indices.size(), 1.0f);
        return ones;
    }

    // edges_ / weights_ / total_weight_ from the entries (v, j) of graph_ above the diagonal that chosen(v, j) picks: once per
    // edge, in entry order, so (lo, hi) ascending, and the weights added one by one in that order
    template <typename Chosen>
    void collect_edges(Chosen chosen) {
        edges_.clear();
        weights_.clear();
        total_weight_ = 0.0;
        for (size_t v = 0; v < matrix_num_rows_; v++)
            for (uint32_t j = graph_.adj_indptr[v]; j < graph_.adj_indptr[v + 1]; j++)
                if (graph_.adj_indices[j] > v && chosen(v, j)) {
                    edges_.push_back(std::make_pair((uint32_t)v, graph_.adj_indices[j]));
                    weights_.push_back(graph_.adj_data[j]);
                    total_weight_ += (double)graph_.adj_data[j];
                }
    }

public:
    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric matrix, weights in adj_data: what results align with

    void send_matrix_host_to_device() {
        PatternApp::send_matrix_host_to_device();
        const size_t nnz = graph_.adj_data.size();
        weight_ = DeviceBuffer(sizeof(float) * (nnz ? nnz : 1));
        if (nnz) weight_.upload(graph_.adj_data.data(), sizeof(float) * nnz);
    }

    double total_weight() const { return total_weight_; }                          // the f64 sum of weights() in entry order
    const std::vector<std::pair<uint32_t, uint32_t>> &edges() const { return edges_; }   // (lo, hi), ascending
    const std::vector<float> &weights() const { return weights_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_PATTERN_APP_H_
