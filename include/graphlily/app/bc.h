// graphlily/app/bc.h -- betweenness centrality over the MI355X backend (an extension: the reference has no such driver), with the
// conventions of the drivers next to it (graphlily/app/kcore.h): print and exit on error, device-resident buffers.
// Brandes' algorithm, one search per source: the search is an app::BFS this object owns, loaded with the simple pattern of the
// matrix (graphlily::io::util_simple_pattern: zero values, the diagonal and duplicates dropped, rows ascending); its levels stay
// on the device, and gl_bc_accumulate (include/graphlily_hip.h) counts the shortest paths level by level through
// that BFS's SpMV plan and adds every vertex's dependency, pulled through the transposed pattern's plan -- a second SpMVModule
// with the (||,&&) semiring, which is loaded only when the pattern is not symmetric.
// Row shards are not supported: the kernel reads the level and the path count of every column of a row.
#ifndef GRAPHLILY_HIP_APP_BC_H_
#define GRAPHLILY_HIP_APP_BC_H_

#include "graphlily/app/bfs.h"
#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <algorithm>
#include <vector>

namespace graphlily {
namespace app {

class BetweennessCentrality : public app::ModuleCollection {
private:
    app::BFS bfs_;
    // the transposed pattern's module: created by the first load that needs two plans (owned by the collection from then on)
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *out_ = nullptr;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    bool runtime_up_ = false;
    uint32_t n_ = 0, n_real_ = 0;
    bool sent_ = false, empty_ = false, directed_ = false, two_plans_ = false;
    std::vector<uint32_t> sources_, depths_, reached_, overflowed_;
    uint32_t orphans_ = 0;

public:
    typedef std::vector<double, aligned_allocator<double>> aligned_bc_vec_t;
    enum Direction { kAuto = -1, kUndirected = 0, kDirected = 1 };

    BetweennessCentrality(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t spmspv_out_buf_len, uint32_t vec_buf_len)
        : bfs_(num_channels, spmv_out_buf_len, spmspv_out_buf_len, vec_buf_len), num_channels_(num_channels),
          spmv_out_buf_len_(spmv_out_buf_len), vec_buf_len_(vec_buf_len) {}

    void set_up_runtime(std::string xclbin_file_path) {
        bfs_.set_target(target_);
        bfs_.set_device(device_);
        bfs_.set_up_runtime(xclbin_file_path);
        ModuleCollection::set_up_runtime(xclbin_file_path);
        runtime_up_ = true;
    }

    uint32_t num_vertices() const { return n_; }            // the padded matrix's
    uint32_t num_real_vertices() const { return n_real_; }
    bool directed() const { return directed_; }

    // direction = kAuto: undirected iff the pattern is symmetric; kUndirected on an asymmetric pattern takes every edge in both
    // directions; kDirected keeps two plans even when the pattern is symmetric
    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, int direction = kAuto) {
        CSRMatrix<float> csr_matrix = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        n_real_ = csr_matrix.num_rows;
        graphlily::io::util_round_csr_matrix_dim(csr_matrix, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        CSRMatrix<float> in, out;
        const bool symmetric = graphlily::io::util_simple_pattern(csr_matrix, in, out);      // after padding
        directed_ = direction == kAuto ? !symmetric : direction == kDirected;
        two_plans_ = directed_;
        if (!directed_ && !symmetric) {
            std::vector<uint32_t> degrees;
            in = graphlily::io::util_symmetrize_simple(csr_matrix, degrees);
        } else if (directed_ && symmetric) {
            out = in;
        }
        n_ = in.num_rows;
        empty_ = in.adj_indices.empty();      // an empty graph: nothing is loaded, run() launches nothing
        if (!empty_) {
            bfs_.load_and_format_matrix(in, skip_empty_rows);
            if (two_plans_) {
                if (!out_) {
                    out_ = new graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t>(num_channels_, spmv_out_buf_len_, vec_buf_len_);
                    out_->set_semiring(graphlily::LogicalSemiring);
                    out_->set_mask_type(graphlily::kNoMask);
                    add_module(out_);
                    if (runtime_up_) {      // what ModuleCollection::set_up_runtime does per module
                        out_->set_device(device_);
                        out_->set_unused_args();
                        out_->set_mode();
                        out_->set_blocking(getenv("GRAPHLILY_BLOCKING") != nullptr && atoi(getenv("GRAPHLILY_BLOCKING")) != 0);
                    }
                }
                out_->load_and_format_matrix(out, skip_empty_rows);
            }
        }
        sent_ = false;
    }

    void send_matrix_host_to_device() {
        if (!empty_) {
            bfs_.send_matrix_host_to_device();
            if (two_plans_) out_->send_matrix_host_to_device();
        }
        sent_ = true;
    }

    // networkx's _rescale for endpoints = false as one factor: n vertices, k sources
    static double scale_of(uint32_t n, size_t k, bool normalized, bool directed) {
        double scale;
        if (normalized) {
            if (n <= 2) return 1.0;
            scale = 1.0 / ((double)(n - 1) * (double)(n - 2));
        } else {
            if (directed) return 1.0;
            scale = 0.5;
        }
        return k < n ? scale * n / k : scale;
    }

    // the betweenness centrality of the padded matrix's vertices (padding vertices: 0) summed over `sources` (real vertices) and
    // scaled as networkx.betweenness_centrality(k = sources.size(), endpoints = false) scales it; the factor is passed to the
    // kernel.  Per source: bfs.pull_push(s, N), N = depth_hint, then gl_bc_accumulate on the levels still on the device.  A search
    // whose deepest level is N + 1 may be truncated: N is doubled, capped at the number of vertices, the source is searched again
    // before anything is accumulated, and the larger N is kept.  Leaves depths(), reached(), orphans() and overflowed() (the
    // sources whose path counts overflowed f64: they contribute nothing and are named on stdout).
    aligned_bc_vec_t run(const std::vector<uint32_t> &sources, bool normalized = false, uint32_t depth_hint = 16) {
        if (!sent_) {
            printf("BetweennessCentrality::run(): send_matrix_host_to_device first\n");
            exit(EXIT_FAILURE);
        }
        for (uint32_t s : sources)
            if (s >= n_real_) {
                printf("BetweennessCentrality::run(): source %u is outside the real vertices 0 .. %u\n", s, n_real_ - 1);
                exit(EXIT_FAILURE);
            }
        sources_ = sources;
        depths_.clear();
        reached_.clear();
        overflowed_.clear();
        orphans_ = 0;
        aligned_bc_vec_t bc(n_, 0.0);
        if (empty_ || sources.empty()) {
            depths_.assign(sources.size(), 1);
            reached_.assign(sources.size(), 1);
            return bc;
        }
        const double scale = scale_of(n_real_, sources.size(), normalized, directed_);
        uint32_t N = std::max<uint32_t>(1, std::min<uint32_t>(depth_hint, n_));
        DeviceBuffer d_bc(sizeof(double) * (size_t)n_);
        for (size_t i = 0; i < sources.size(); i++) {
            float deepest = 0;
            for (;;) {
                auto level = bfs_.pull_push(sources[i], N);
                deepest = 0;
                for (float l : level) deepest = std::max(deepest, l);
                if ((uint32_t)deepest < N + 1 || N >= n_) break;
                N = (uint32_t)std::min<uint64_t>(2ull * N, n_);
            }
            uint32_t stats[4] = {0, 0, 0, 0};
            bfs_.spmv_module()->bc_accumulate(two_plans_ ? out_ : nullptr, bfs_.last_levels(), d_bc, scale, i > 0, nullptr, stats);
            if (stats[0] != (uint32_t)deepest) {
                printf("BetweennessCentrality::run(): gl_bc_accumulate saw depth %u, the search from %u returned depth %u\n", stats[0],
                       sources[i], (uint32_t)deepest);
                exit(EXIT_FAILURE);
            }
            depths_.push_back(stats[0]);
            reached_.push_back(stats[1]);
            orphans_ += stats[2];
            if (stats[3]) {
                overflowed_.push_back(sources[i]);
                printf("BetweennessCentrality::run(): the shortest-path counts of the search from %u overflowed f64; it contributes nothing\n",
                       sources[i]);
            }
        }
        d_bc.download(bc.data(), sizeof(double) * (size_t)n_);
        return bc;
    }
    aligned_bc_vec_t run(bool normalized = false, uint32_t depth_hint = 16) {      // all real vertices
        std::vector<uint32_t> all(n_real_);
        for (uint32_t v = 0; v < n_real_; v++) all[v] = v;
        return run(all, normalized, depth_hint);
    }
    const std::vector<uint32_t> &sources() const { return sources_; }
    const std::vector<uint32_t> &depths() const { return depths_; }             // per source: the deepest level
    const std::vector<uint32_t> &reached() const { return reached_; }           // per source: the vertices of level >= 1
    const std::vector<uint32_t> &overflowed() const { return overflowed_; }
    uint32_t orphans() const { return orphans_; }                               // 0: the levels are BFS results
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_BC_H_
