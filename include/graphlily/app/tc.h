// graphlily/app/tc.h -- triangle counting over the MI355X backend (an extension: the reference has no such driver), with the
// conventions of the drivers next to it (graphlily/app/cc.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_tc_count walks
// (include/graphlily_hip.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and oriented by degree on the host (graphlily::io::util_triangle_orient): row v
// keeps the neighbours u with (deg[u], u) > (deg[v], v), so every triangle is found exactly once and hub rows are short.
//   triangles[v] = triangles through v
// Row shards are not supported: the kernel reads row u for every column u of a row.
#ifndef GRAPHLILY_HIP_APP_TC_H_
#define GRAPHLILY_HIP_APP_TC_H_

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <vector>

namespace graphlily {
namespace app {

class TriangleCount : public app::ModuleCollection {
private:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *SpMV_;
    uint32_t matrix_num_rows_ = 0, matrix_num_cols_ = 0;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    graphlily::SemiringType semiring_ = graphlily::LogicalSemiring;
    uint32_t n_real_ = 0;
    bool sent_ = false;
    std::vector<uint32_t> degrees_;
    uint64_t num_triangles_ = 0, num_wedges_ = 0;

public:
    typedef std::vector<uint64_t, aligned_allocator<uint64_t>> aligned_count_vec_t;

    TriangleCount(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : num_channels_(num_channels), spmv_out_buf_len_(spmv_out_buf_len), vec_buf_len_(vec_buf_len) {
        SpMV_ = new graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t>(num_channels_, spmv_out_buf_len_, vec_buf_len_);
        SpMV_->set_semiring(semiring_);
        SpMV_->set_mask_type(graphlily::kNoMask);
        add_module(SpMV_);
    }

    uint32_t get_nnz() { return SpMV_->get_nnz(); }                 // entries of the oriented matrix: the undirected edges
    uint32_t num_vertices() const { return matrix_num_rows_; }      // the padded matrix's
    uint32_t num_real_vertices() const { return n_real_; }
    const std::vector<uint32_t> &degrees() const { return degrees_; }

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows) {
        CSRMatrix<float> csr_matrix = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        n_real_ = csr_matrix.num_rows;
        graphlily::io::util_round_csr_matrix_dim(csr_matrix, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        CSRMatrix<float> oriented = graphlily::io::util_triangle_orient(csr_matrix, degrees_);      // after padding
        SpMV_->load_and_format_matrix(oriented, skip_empty_rows);
        matrix_num_rows_ = SpMV_->get_num_rows();
        matrix_num_cols_ = SpMV_->get_num_cols();
        assert(matrix_num_rows_ == matrix_num_cols_);
        num_wedges_ = 0;
        for (uint64_t d : degrees_) num_wedges_ += d * (d - (d ? 1 : 0)) / 2;
        sent_ = false;
    }

    void send_matrix_host_to_device() {
        SpMV_->send_matrix_host_to_device();
        sent_ = true;
    }

    // triangles through every vertex of the padded matrix (padding vertices: 0); leaves num_triangles() and transitivity()
    aligned_count_vec_t run() {
        if (!sent_) {
            printf("TriangleCount::run(): send_matrix_host_to_device first\n");
            exit(EXIT_FAILURE);
        }
        const uint32_t n = matrix_num_rows_;
        DeviceBuffer out(sizeof(uint64_t) * ((size_t)n + 1));       // 64-bit words: the total, then the per-vertex counts
        SpMV_->tc_count(out, (uint64_t *)out.ptr() + 1);
        aligned_count_vec_t counts((size_t)n + 1);
        out.download(counts.data(), sizeof(uint64_t) * ((size_t)n + 1));
        num_triangles_ = counts[0];                                 // (the orientation gives every triangle once)
        counts.erase(counts.begin());
        return counts;
    }
    uint64_t num_triangles() const { return num_triangles_; }
    uint64_t num_wedges() const { return num_wedges_; }
    double transitivity() const { return num_wedges_ ? 3.0 * (double)num_triangles_ / (double)num_wedges_ : 0.0; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_TC_H_
