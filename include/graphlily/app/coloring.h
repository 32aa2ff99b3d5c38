// graphlily/app/coloring.h -- graph colouring over the MI355X backend (an extension: the reference has no such driver), with the
// conventions of the drivers next to it (graphlily/app/kcore.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_color walks
// (include/graphlily_hip_ext.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and stored in both directions by the host
// (graphlily::io::util_symmetrize_simple): colouring v must reach every neighbour of v through row v.
//   colour[v] = the smallest non-negative integer that no neighbour going before v has; u goes before v iff prio[u] > prio[v], or
//               they are equal and u < v: the sequential first-fit greedy colouring in that order, to the bit
// Row shards are not supported: the kernel reads row u for every column u of a row.
#ifndef GRAPHLILY_HIP_APP_COLORING_H_
#define GRAPHLILY_HIP_APP_COLORING_H_

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <string>
#include <vector>

namespace graphlily {
namespace app {

class GraphColoring : public app::ModuleCollection {
private:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *SpMV_;
    uint32_t matrix_num_rows_ = 0, matrix_num_cols_ = 0;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    graphlily::SemiringType semiring_ = graphlily::LogicalSemiring;
    uint32_t n_real_ = 0;
    bool sent_ = false;
    std::vector<uint32_t> degrees_, priorities_;
    std::vector<uint64_t> color_sizes_;
    uint64_t num_colors_ = 0, rounds_ = 0, launches_ = 0, widest_ = 0;
    uint32_t degeneracy_ = 0;

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_color_vec_t;

    GraphColoring(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
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

    // colours of the padded matrix's vertices (padding vertices: 0) in the order graphlily::io::util_coloring_priorities gives
    // for "natural", "random", "largest_first" or "smallest_last" (which first runs gl_kcore on the same plan for its peeling
    // order and then needs at most degeneracy() + 1 colours); leaves num_colors(), rounds(), launches(), widest(), color_sizes()
    // and priorities(): the array the run used (empty for "natural").  The call waits for the device.
    aligned_color_vec_t run(std::string order = "largest_first", uint32_t seed = 0) {
        if (!sent_) {
            printf("GraphColoring::run(): send_matrix_host_to_device first\n");
            exit(EXIT_FAILURE);
        }
        const size_t n = matrix_num_rows_;
        degeneracy_ = 0;
        if (order == "smallest_last") {
            DeviceBuffer peel(sizeof(uint32_t) * 2 * n);             // the core numbers, then the order
            uint32_t kstats[4] = {0, 0, 0, 0};
            SpMV_->kcore(peel, (uint32_t *)peel.ptr() + n, kstats);
            std::vector<uint32_t> words(2 * n);
            peel.download(words.data(), sizeof(uint32_t) * 2 * n);
            degeneracy_ = kstats[0];
            priorities_ = graphlily::io::util_coloring_priorities(degrees_, order, seed, std::vector<uint32_t>(words.begin() + n, words.end()));
        } else {
            priorities_ = graphlily::io::util_coloring_priorities(degrees_, order, seed);
        }
        const bool with_prio = !priorities_.empty();
        DeviceBuffer out(sizeof(uint32_t) * (with_prio ? 2 * n : n));       // the colours, then the priorities
        if (with_prio) GRAPHLILY_CHECK(gl_buf_h2d((uint32_t *)out.ptr() + n, priorities_.data(), sizeof(uint32_t) * n));
        uint64_t stats[4] = {0, 0, 0, 0};
        SpMV_->color(out, with_prio ? (const uint32_t *)out.ptr() + n : nullptr, stats);
        aligned_color_vec_t color(n);
        out.download(color.data(), sizeof(uint32_t) * n);
        num_colors_ = stats[0];
        rounds_ = stats[1];
        launches_ = stats[2];
        widest_ = stats[3];
        color_sizes_.assign((size_t)num_colors_, 0);
        for (uint32_t v = 0; v < n_real_; v++)
            if (color[v] < num_colors_) color_sizes_[color[v]]++;
        return color;
    }
    uint64_t num_colors() const { return num_colors_; }
    uint64_t rounds() const { return rounds_; }
    uint64_t launches() const { return launches_; }
    uint64_t widest() const { return widest_; }
    uint32_t degeneracy() const { return degeneracy_; }                         // of the last "smallest_last" run
    const std::vector<uint32_t> &priorities() const { return priorities_; }     // empty for "natural"
    const std::vector<uint64_t> &color_sizes() const { return color_sizes_; }   // [c] = real vertices of colour c
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_COLORING_H_
