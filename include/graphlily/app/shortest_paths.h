// graphlily/app/shortest_paths.h -- weighted shortest paths run to convergence over the MI355X backend (an extension: the
// reference's SSSP is Bellman-Ford for a number of iterations its caller guesses), with the conventions of the drivers next to it
// (graphlily/app/topo.h): print and exit on error, device-resident buffers.  The matrix is read as a DIRECTED graph
// (graphlily::io::util_directed_weighted with keep_smallest: an edge u -> v for a stored entry A[v,u], u != v, parallel edges
// collapse to the shortest; weighted = false gives every edge the weight 1 and takes a stored zero for no edge); negative, NaN
// and infinite weights are refused.  One SpMVModule with the (||,&&) semiring holds the pattern, a second one the transposed
// pattern when the pattern is not symmetric (PatternApp::load_transposed); the weights travel in buffers of their own, aligned
// with graph().adj_indices and graph_out().adj_indices.  gl_sssp_delta (include/graphlily_hip_sssp_delta.h):
//   dist[v]   = Dijkstra's f32 result to the bit, whatever delta; +inf when unreached
//   parent[v] = v on a source, the smallest u with d[u] < d[v] and (float)(d[u] + w) == d[v] elsewhere, 0xffffffff without one
// Row shards are not supported: the kernel lowers the distance of every column of a row of the transposed pattern.
#ifndef GRAPHLILY_HIP_APP_SHORTEST_PATHS_H_
#define GRAPHLILY_HIP_APP_SHORTEST_PATHS_H_

#include "graphlily/app/pattern_app.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace graphlily {
namespace app {

class ShortestPaths : public app::PatternApp {
private:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *out_ = nullptr;      // (PatternApp::load_transposed)
    CSRMatrix<float> graph_, graph_out_;
    DeviceBuffer weight_, weight_out_;
    bool runtime_up_ = false, symmetric_ = true, weighted_ = true;
    std::vector<float> dist_;
    std::vector<uint32_t> parent_;
    uint64_t reached_ = 0, orphans_ = 0, buckets_ = 0, rounds_ = 0, relaxations_ = 0, launches_ = 0;
    float delta_ = 0.0f;

    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        if (weighted_)
            for (uint32_t v = 0; v < padded.num_rows; v++)
                for (uint32_t i = padded.adj_indptr[v]; i < padded.adj_indptr[v + 1]; i++) {
                    const float w = padded.adj_data[i];
                    if (padded.adj_indices[i] != v && !(w >= 0.0f && w - w == 0.0f)) {
                        printf("ShortestPaths: entry %u (%u, %u) is %g: delta-stepping needs finite weights >= 0\n", i, v, padded.adj_indices[i], (double)w);
                        exit(EXIT_FAILURE);
                    }
                }
        symmetric_ = graphlily::io::util_directed_weighted(padded, graph_, graph_out_, weighted_, true);
        return ones_of(graph_);
    }

public:
    typedef std::vector<float, aligned_allocator<float>> aligned_dist_vec_t;

    ShortestPaths(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("ShortestPaths", num_channels, spmv_out_buf_len, vec_buf_len) {}

    void set_up_runtime(std::string xclbin_file_path) {
        ModuleCollection::set_up_runtime(xclbin_file_path);
        runtime_up_ = true;
    }

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, bool weighted = true) {
        weighted_ = weighted;
        PatternApp::load_and_format_matrix(csr_float_npz_path, skip_empty_rows);      // (calls prepare())
        if (!symmetric_) load_transposed(out_, graph_out_, skip_empty_rows, runtime_up_);
    }

    void send_matrix_host_to_device() {
        PatternApp::send_matrix_host_to_device();
        if (!symmetric_) out_->send_matrix_host_to_device();
        weight_ = upload_weights(graph_);
        weight_out_ = upload_weights(graph_out());
    }

    // 32 * mean weight / mean out-degree over the real vertices; +inf when every weight is 0 or there is no edge (a labelled guess)
    float default_delta() const {
        const size_t nnz = graph_.adj_data.size();
        double sum = 0.0;
        for (float w : graph_.adj_data) sum += (double)w;
        const float delta = nnz && n_real_ ? (float)(32.0 * (sum / (double)nnz) * (double)n_real_ / (double)nnz) : 0.0f;
        return delta > 0.0f && delta - delta == 0.0f ? delta : std::numeric_limits<float>::infinity();
    }

    // distances of the padded matrix's vertices from the nearest of `sources` (padding vertices are isolated); delta <= 0 takes
    // default_delta().  Leaves dist(), reached(), buckets(), rounds(), relaxations(), launches(), delta() and, with want_parents,
    // parent() and orphans().  The call waits for the device.
    aligned_dist_vec_t run(std::vector<uint32_t> const &sources, float delta = 0.0f, bool want_parents = true) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, room = n ? n : 1, k = sources.size();
        for (uint32_t s : sources)
            if (s >= n) { printf("ShortestPaths::run: source %u of %zu vertices\n", s, n); exit(EXIT_FAILURE); }
        delta_ = delta > 0.0f ? delta : default_delta();
        DeviceBuffer out(sizeof(uint32_t) * 2 * room), src(sizeof(uint32_t) * (k ? k : 1));      // dist, parent; the sources
        if (k) src.upload(sources.data(), sizeof(uint32_t) * k);
        uint64_t stats[5] = {0, 0, 0, 0, 0};
        SpMV_->sssp_delta(symmetric_ ? nullptr : out_, (const float *)weight_.ptr(), (const float *)weight_out_.ptr(), (const uint32_t *)src.ptr(),
                          (uint32_t)k, delta_, out, want_parents ? (uint32_t *)out.ptr() + room : nullptr, stats);
        std::vector<uint32_t> got(2 * room);
        out.download(got.data(), sizeof(uint32_t) * 2 * room);
        dist_.resize(n);
        memcpy(dist_.data(), got.data(), sizeof(float) * n);
        parent_.clear();
        orphans_ = 0;
        if (want_parents) {
            parent_.assign(got.begin() + room, got.begin() + room + n);
            for (size_t v = 0; v < n; v++) orphans_ += std::isfinite(dist_[v]) && parent_[v] == 0xffffffffu;
        }
        reached_ = stats[0];
        buckets_ = stats[1];
        rounds_ = stats[2];
        relaxations_ = stats[3];
        launches_ = stats[4];
        return aligned_dist_vec_t(dist_.begin(), dist_.end());
    }

    // v, parent()[v], ... back to a source of the last run (or to an orphan); empty when v is unreached or no parents were asked for
    std::vector<uint32_t> path(uint32_t v) const {
        std::vector<uint32_t> path;
        if (parent_.empty() || v >= dist_.size() || !std::isfinite(dist_[v])) return path;
        path.push_back(v);
        while (parent_[path.back()] != path.back() && parent_[path.back()] != 0xffffffffu) path.push_back(parent_[path.back()]);
        return path;
    }

    const CSRMatrix<float> &graph() const { return graph_; }                    // row v: the predecessors of v (weights in adj_data)
    const CSRMatrix<float> &graph_out() const { return symmetric_ && !weighted_ ? graph_ : graph_out_; }      // row u: its successors
    bool symmetric() const { return symmetric_; }
    const std::vector<float> &dist() const { return dist_; }
    const std::vector<uint32_t> &parent() const { return parent_; }             // empty unless run(.., .., true)
    uint64_t reached() const { return reached_; }
    uint64_t orphans() const { return orphans_; }
    uint64_t buckets() const { return buckets_; }
    uint64_t rounds() const { return rounds_; }
    uint64_t relaxations() const { return relaxations_; }
    uint64_t launches() const { return launches_; }
    float delta() const { return delta_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_SHORTEST_PATHS_H_
