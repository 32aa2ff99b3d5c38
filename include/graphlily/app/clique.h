// graphlily/app/clique.h -- k-clique counting, 3 <= k <= 8, over the MI355X backend (an extension: the reference has no such
// driver), with the conventions of the drivers next to it (graphlily/app/tc.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_clique_count walks
// (include/graphlily_hip_clique.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and oriented by a rank on the host (graphlily::io::util_orient_by_rank): row v
// keeps the neighbours u with (rank[u], u) > (rank[v], v), so every k-clique is found exactly once, from its lowest-ranked vertex.
//   cliques[v] = k-cliques through v
// set_rank() before load_and_format_matrix chooses the rank (one word per vertex of the PADDED matrix; empty, the default: the
// degrees, TriangleCount's orientation).  The kernel refuses rows above 8192 entries; a vertex's position in a degeneracy ordering
// (KCore::run(true), then position[order()[i]] = i) bounds every row by the degeneracy.
// Row shards are not supported: the kernel reads row u for every column u of a row.
#ifndef GRAPHLILY_HIP_APP_CLIQUE_H_
#define GRAPHLILY_HIP_APP_CLIQUE_H_

#include "graphlily/app/pattern_app.h"

#include <vector>

namespace graphlily {
namespace app {

class CliqueCount : public app::PatternApp {
private:
    std::vector<uint32_t> rank_;
    uint64_t num_cliques_ = 0, bins_[4] = {0, 0, 0, 0};
    uint32_t k_ = 0;

    // get_nnz() counts the entries of the oriented matrix: the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        return graphlily::io::util_orient_by_rank(padded, rank_, degrees_);
    }

public:
    typedef std::vector<uint64_t, aligned_allocator<uint64_t>> aligned_count_vec_t;

    CliqueCount(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("CliqueCount", num_channels, spmv_out_buf_len, vec_buf_len) {}

    void set_rank(std::vector<uint32_t> const &rank) { rank_ = rank; }

    // k-cliques through every vertex of the padded matrix (padding vertices: 0); leaves num_cliques(), k() and bins()
    aligned_count_vec_t run(uint32_t k) {
        require_sent("run()");
        const uint32_t n = matrix_num_rows_;
        DeviceBuffer out(sizeof(uint64_t) * ((size_t)n + 1));       // 64-bit words: the total, then the per-vertex counts
        SpMV_->clique_count(k, out, (uint64_t *)out.ptr() + 1, bins_);
        aligned_count_vec_t counts((size_t)n + 1);
        out.download(counts.data(), sizeof(uint64_t) * ((size_t)n + 1));
        num_cliques_ = counts[0];                                   // (the orientation gives every clique once)
        k_ = k;
        counts.erase(counts.begin());
        return counts;
    }
    // the number of k-cliques alone: kernels without the per-vertex bookkeeping
    uint64_t run_total(uint32_t k) {
        require_sent("run_total()");
        DeviceBuffer out(sizeof(uint64_t));
        SpMV_->clique_count(k, out, nullptr, bins_);
        out.download(&num_cliques_, sizeof(uint64_t));
        k_ = k;
        return num_cliques_;
    }
    uint64_t num_cliques() const { return num_cliques_; }
    uint32_t k() const { return k_; }
    const uint64_t *bins() const { return bins_; }       // rows in the tiny and mid bins, the wide bin, the long bin; launches
    // num_cliques() / C(real vertices, k), 0.0 where there is no k-subset
    double clique_density() const {
        double subsets = 1.0;
        for (uint32_t i = 0; i < k_; i++) subsets *= ((double)n_real_ - i) / (double)(i + 1);
        return k_ && subsets > 0.0 ? (double)num_cliques_ / subsets : 0.0;
    }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_CLIQUE_H_
