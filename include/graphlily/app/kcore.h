// graphlily/app/kcore.h -- k-core decomposition over the MI355X backend (an extension: the reference has no such driver), with
// the conventions of the drivers next to it (graphlily/app/tc.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_kcore peels
// (include/graphlily_hip.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and stored in both directions by the host
// (graphlily::io::util_symmetrize_simple): peeling v must reach every neighbour of v through row v.
//   core[v] = the largest k such that v lies in a subgraph in which every vertex has degree >= k
// Row shards are not supported: the kernel reads row u for every column u of a row.
#ifndef GRAPHLILY_HIP_APP_KCORE_H_
#define GRAPHLILY_HIP_APP_KCORE_H_

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <vector>

namespace graphlily {
namespace app {

class KCore : public app::ModuleCollection {
private:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *SpMV_;
    uint32_t matrix_num_rows_ = 0, matrix_num_cols_ = 0;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    graphlily::SemiringType semiring_ = graphlily::LogicalSemiring;
    uint32_t n_real_ = 0;
    bool sent_ = false;
    std::vector<uint32_t> degrees_, order_;
    std::vector<uint64_t> core_sizes_;
    uint32_t degeneracy_ = 0, levels_ = 0, sub_rounds_ = 0, launches_ = 0;

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_core_vec_t;

    KCore(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
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

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows) {
        CSRMatrix<float> csr_matrix = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        n_real_ = csr_matrix.num_rows;
        graphlily::io::util_round_csr_matrix_dim(csr_matrix, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        CSRMatrix<float> sym = graphlily::io::util_symmetrize_simple(csr_matrix, degrees_);      // after padding
        SpMV_->load_and_format_matrix(sym, skip_empty_rows);
        matrix_num_rows_ = SpMV_->get_num_rows();
        matrix_num_cols_ = SpMV_->get_num_cols();
        assert(matrix_num_rows_ == matrix_num_cols_);
        sent_ = false;
    }

    void send_matrix_host_to_device() {
        SpMV_->send_matrix_host_to_device();
        sent_ = true;
    }

    // core numbers of the padded matrix's vertices (padding vertices: 0); leaves degeneracy(), levels(), sub_rounds(),
    // core_sizes() and, with want_order, order(): a degeneracy ordering (not unique).  The call waits for the device.
    aligned_core_vec_t run(bool want_order = false) {
        if (!sent_) {
            printf("KCore::run(): send_matrix_host_to_device first\n");
            exit(EXIT_FAILURE);
        }
        const size_t n = matrix_num_rows_, words = want_order ? 2 * n : n;
        DeviceBuffer out(sizeof(uint32_t) * words);                  // the core numbers, then the order
        uint32_t stats[4] = {0, 0, 0, 0};
        SpMV_->kcore(out, want_order ? (uint32_t *)out.ptr() + n : nullptr, stats);
        aligned_core_vec_t core(words);
        out.download(core.data(), sizeof(uint32_t) * words);
        order_.assign(core.begin() + n, core.end());
        core.resize(n);
        degeneracy_ = stats[0];
        levels_ = stats[1];
        sub_rounds_ = stats[2];
        launches_ = stats[3];
        std::vector<uint64_t> count((size_t)degeneracy_ + 2, 0);
        for (uint32_t v = 0; v < n_real_; v++) count[core[v] <= degeneracy_ ? core[v] : degeneracy_ + 1]++;
        core_sizes_.assign((size_t)degeneracy_ + 1, 0);
        uint64_t above = count[(size_t)degeneracy_ + 1];
        for (size_t k = (size_t)degeneracy_ + 1; k-- > 0;) core_sizes_[k] = above += count[k];
        return core;
    }
    uint32_t degeneracy() const { return degeneracy_; }
    uint32_t levels() const { return levels_; }
    uint32_t sub_rounds() const { return sub_rounds_; }
    uint32_t launches() const { return launches_; }
    const std::vector<uint32_t> &order() const { return order_; }               // empty unless run(true)
    const std::vector<uint64_t> &core_sizes() const { return core_sizes_; }     // [k] = real vertices with core >= k
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_KCORE_H_
