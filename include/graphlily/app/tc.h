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

#include "graphlily/app/pattern_app.h"

#include <vector>

namespace graphlily {
namespace app {

class TriangleCount : public app::PatternApp {
private:
    uint64_t num_triangles_ = 0, num_wedges_ = 0;

    // get_nnz() counts the entries of the oriented matrix: the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        CSRMatrix<float> oriented = graphlily::io::util_triangle_orient(padded, degrees_);
        num_wedges_ = 0;
        for (uint64_t d : degrees_) num_wedges_ += d * (d - (d ? 1 : 0)) / 2;
        return oriented;
    }

public:
    typedef std::vector<uint64_t, aligned_allocator<uint64_t>> aligned_count_vec_t;

    TriangleCount(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("TriangleCount", num_channels, spmv_out_buf_len, vec_buf_len) {}

    // triangles through every vertex of the padded matrix (padding vertices: 0); leaves num_triangles() and transitivity()
    aligned_count_vec_t run() {
        require_sent("run()");
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
