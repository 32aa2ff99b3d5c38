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

#include "graphlily/app/pattern_app.h"

#include <string>
#include <vector>

namespace graphlily {
namespace app {

class GraphColoring : public app::PatternApp {
private:
    std::vector<uint32_t> priorities_;
    std::vector<uint64_t> color_sizes_;
    uint64_t num_colors_ = 0, rounds_ = 0, launches_ = 0, widest_ = 0;
    uint32_t degeneracy_ = 0;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        return graphlily::io::util_symmetrize_simple(padded, degrees_);
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_color_vec_t;

    GraphColoring(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("GraphColoring", num_channels, spmv_out_buf_len, vec_buf_len) {}

    // colours of the padded matrix's vertices (padding vertices: 0) in the order graphlily::io::util_coloring_priorities gives
    // for "natural", "random", "largest_first" or "smallest_last" (which first runs gl_kcore on the same plan for its peeling
    // order and then needs at most degeneracy() + 1 colours); leaves num_colors(), rounds(), launches(), widest(), color_sizes()
    // and priorities(): the array the run used (empty for "natural").  The call waits for the device.
    aligned_color_vec_t run(std::string order = "largest_first", uint32_t seed = 0) {
        require_sent("run()");
        const size_t n = matrix_num_rows_;
        degeneracy_ = 0;
        if (order == "smallest_last")
            priorities_ = graphlily::io::util_coloring_priorities(degrees_, order, seed, peel_order(&degeneracy_));
        else
            priorities_ = graphlily::io::util_coloring_priorities(degrees_, order, seed);
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
