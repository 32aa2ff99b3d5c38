// graphlily/app/closeness.h -- closeness and harmonic centrality, eccentricities and hop distances over the MI355X backend (an
// extension: the reference has no such driver), with the conventions of the drivers next to it (graphlily/app/scc.h): print and
// exit on error, device-resident buffers.  The matrix is read as a simple DIRECTED graph (graphlily::io::util_simple_pattern: an
// edge u -> v for a stored non-zero A[v,u], u != v).  One SpMVModule with the (||,&&) semiring holds the pattern, so that the plan
// is the boolean layout, whose plain row copy gl_msbfs walks (include/graphlily_hip_msbfs.h); a second one holds
// the transposed pattern and is loaded only when the pattern is not symmetric, as in graphlily/app/scc.h and topo.h.
//   far[v], reach[v] = the sum and the number of the finite distances >= 1 between v and the sources; harmonic[v] = the sum of
//   their reciprocals, per batch of 64 sources level by level ascending; closeness[v] = reach / far, times reach / (n_real - 1)
//   with wf_improved -- networkx.closeness_centrality when every vertex is a source.
// reverse = false sums at every vertex its INCOMING distances d(s, v), networkx's convention on a DiGraph; reverse = true walks
// the transposed pattern's plan.  Row shards are not supported: the kernel reads the frontier word of every column of a row.
#ifndef GRAPHLILY_HIP_APP_CLOSENESS_H_
#define GRAPHLILY_HIP_APP_CLOSENESS_H_

#include "graphlily/app/pattern_app.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace graphlily {
namespace app {

class ClosenessCentrality : public app::PatternApp {
private:
    // the transposed pattern's module: created by the first load that needs two plans (owned by the collection from then on)
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *out_ = nullptr;
    CSRMatrix<float> graph_, graph_out_;
    bool runtime_up_ = false, symmetric_ = true;
    std::vector<uint64_t> far_, source_reach_, source_far_, eccentricity_;
    std::vector<uint32_t> reach_, hops_, sources_, center_, periphery_;
    std::vector<double> harmonic_, closeness_;
    uint64_t batches_ = 0, levels_ = 0, launches_ = 0, diameter_ = 0, radius_ = 0;

    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        symmetric_ = graphlily::io::util_simple_pattern(padded, graph_, graph_out_);
        return graph_;
    }

public:
    static const uint32_t kBatch = 64;

    ClosenessCentrality(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("ClosenessCentrality", num_channels, spmv_out_buf_len, vec_buf_len) {}

    void set_up_runtime(std::string xclbin_file_path) {
        ModuleCollection::set_up_runtime(xclbin_file_path);
        runtime_up_ = true;
    }

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows) {
        PatternApp::load_and_format_matrix(csr_float_npz_path, skip_empty_rows);      // (calls prepare())
        if (symmetric_) return;
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
        out_->load_and_format_matrix(graph_out_, skip_empty_rows);
    }

    void send_matrix_host_to_device() {
        PatternApp::send_matrix_host_to_device();
        if (!symmetric_) out_->send_matrix_host_to_device();
    }

    // the closeness of the padded matrix's vertices (padding vertices: 0) with respect to `sources` -- distinct real vertices, dealt
    // in the given order into batches of 64, one gl_msbfs call each, accumulating from the second on; an EMPTY list means every
    // real vertex.  Leaves far(), reach(), harmonic(), closeness(), sources(), batches(), levels(), launches(), per source
    // eccentricity(), source_reach() and source_far(), diameter() (exact when every vertex is a source, else a lower bound),
    // radius(), center(), periphery() and, with want_hops, hops() (sources x num_vertices words).  The call waits for the device.
    std::vector<double> run(std::vector<uint32_t> sources = std::vector<uint32_t>(), bool reverse = false, bool wf_improved = true,
                            bool want_hops = false) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, room = n ? n : 1;
        if (sources.empty())
            for (uint32_t v = 0; v < n_real_; v++) sources.push_back(v);
        std::vector<bool> given(n_real_, false);
        for (uint32_t s : sources) {
            if (s >= n_real_ || given[s]) {
                printf("%s::run(): source %u is %s\n", name_, s, s >= n_real_ ? "no real vertex" : "given twice");
                exit(EXIT_FAILURE);
            }
            given[s] = true;
        }
        sources_ = sources;
        const size_t k_all = sources.size(), k_most = std::min<size_t>(kBatch, std::max<size_t>(1, k_all));
        DeviceBuffer far(sizeof(uint64_t) * room), harmonic(sizeof(double) * room), reach(sizeof(uint32_t) * room);
        DeviceBuffer hops(sizeof(uint32_t) * (want_hops ? k_most * room : 1));
        graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *walk = reverse && !symmetric_ ? out_ : SpMV_;
        batches_ = levels_ = launches_ = 0;
        source_reach_.assign(k_all, 0);
        source_far_.assign(k_all, 0);
        eccentricity_.assign(k_all, 0);
        hops_.assign(want_hops ? k_all * n : 0, 0);
        for (size_t b = 0; b < k_all; b += kBatch) {
            const uint32_t k = (uint32_t)std::min<size_t>(kBatch, k_all - b);
            uint64_t source_stats[3 * kBatch], stats[4] = {0, 0, 0, 0};
            walk->msbfs(sources.data() + b, k, b > 0, far, reach, harmonic, want_hops ? (uint32_t *)hops.ptr() : nullptr, source_stats, stats);
            for (uint32_t j = 0; j < k; j++) {
                source_reach_[b + j] = source_stats[3 * j];
                source_far_[b + j] = source_stats[3 * j + 1];
                eccentricity_[b + j] = source_stats[3 * j + 2];
            }
            batches_++;
            levels_ += stats[0];
            launches_ += stats[2];
            if (want_hops && n) hops.download(hops_.data() + b * n, sizeof(uint32_t) * k * n);
        }
        far_.assign(n, 0);
        reach_.assign(n, 0);
        harmonic_.assign(n, 0.0);
        if (k_all && n) {
            far.download(far_.data(), sizeof(uint64_t) * n);
            reach.download(reach_.data(), sizeof(uint32_t) * n);
            harmonic.download(harmonic_.data(), sizeof(double) * n);
        }
        diameter_ = radius_ = 0;
        center_.clear();
        periphery_.clear();
        if (k_all) {
            diameter_ = *std::max_element(eccentricity_.begin(), eccentricity_.end());
            radius_ = *std::min_element(eccentricity_.begin(), eccentricity_.end());
            for (size_t j = 0; j < k_all; j++) {
                if (eccentricity_[j] == radius_) center_.push_back(sources[j]);
                if (eccentricity_[j] == diameter_) periphery_.push_back(sources[j]);
            }
        }
        closeness_.assign(n, 0.0);
        for (size_t v = 0; v < n; v++) {
            if (!far_[v]) continue;
            double c = (double)reach_[v] / (double)far_[v];
            if (wf_improved) c = n_real_ > 1 ? c * ((double)reach_[v] / (double)(n_real_ - 1)) : 0.0;
            closeness_[v] = c;
        }
        return closeness_;
    }

    const CSRMatrix<float> &graph() const { return graph_; }                    // row v: the predecessors of v
    const CSRMatrix<float> &graph_out() const { return symmetric_ ? graph_ : graph_out_; }      // row v: its successors
    bool symmetric() const { return symmetric_; }
    const std::vector<uint64_t> &far() const { return far_; }
    const std::vector<uint32_t> &reach() const { return reach_; }
    const std::vector<double> &harmonic() const { return harmonic_; }
    const std::vector<double> &closeness() const { return closeness_; }
    const std::vector<uint32_t> &hops() const { return hops_; }                 // empty unless run(.., want_hops = true)
    const std::vector<uint32_t> &sources() const { return sources_; }
    const std::vector<uint64_t> &eccentricity() const { return eccentricity_; } // per source, as the next two
    const std::vector<uint64_t> &source_reach() const { return source_reach_; }
    const std::vector<uint64_t> &source_far() const { return source_far_; }
    const std::vector<uint32_t> &center() const { return center_; }
    const std::vector<uint32_t> &periphery() const { return periphery_; }
    uint64_t diameter() const { return diameter_; }
    uint64_t radius() const { return radius_; }
    uint64_t batches() const { return batches_; }
    uint64_t levels() const { return levels_; }
    uint64_t launches() const { return launches_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_CLOSENESS_H_
