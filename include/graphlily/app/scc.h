// graphlily/app/scc.h -- strongly connected components over the MI355X backend (an extension: the reference has no such driver),
// with the conventions of the drivers next to it (graphlily/app/coloring.h): print and exit on error, device-resident buffers.
// The matrix is read as a simple DIRECTED graph (graphlily::io::util_simple_pattern: an edge u -> v for a stored non-zero A[v,u],
// u != v; zero values, the diagonal and duplicates dropped, rows ascending).  One SpMVModule with the (||,&&) semiring holds the
// pattern, so that the plan is the boolean layout, whose plain row copy gl_scc walks (include/graphlily_hip_scc.h, DESIGN.md
// 4.22); a second one holds the transposed pattern and is loaded only when the pattern is not symmetric, as in graphlily/app/bc.h.
//   label[v] = the smallest vertex u such that v reaches u and u reaches v: unique, app::ConnectedComponents' convention
// Row shards are not supported: the kernel reads the colour of every column of a row, in the pattern and in its transpose.
#ifndef GRAPHLILY_HIP_APP_SCC_H_
#define GRAPHLILY_HIP_APP_SCC_H_

#include "graphlily/app/pattern_app.h"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace graphlily {
namespace app {

class StronglyConnectedComponents : public app::PatternApp {
private:
    // the transposed pattern's module: created by the first load that needs two plans (owned by the collection from then on)
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *out_ = nullptr;
    CSRMatrix<float> graph_, graph_out_;
    bool runtime_up_ = false, symmetric_ = true;
    std::vector<uint32_t> labels_, priorities_, component_labels_;
    std::vector<uint64_t> component_sizes_;
    uint64_t num_components_ = 0, largest_component_ = 0, passes_ = 0, trimmed_ = 0, rounds_ = 0, launches_ = 0;

    // get_nnz() counts the edges of the simple directed graph; degrees_ = in-degree + out-degree
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        symmetric_ = graphlily::io::util_simple_pattern(padded, graph_, graph_out_);
        degrees_.assign(graph_.num_rows, 0);
        for (uint32_t v = 0; v < graph_.num_rows; v++) degrees_[v] = graph_.adj_indptr[v + 1] - graph_.adj_indptr[v];
        for (uint32_t u : graph_.adj_indices) degrees_[u]++;
        return graph_;
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_label_vec_t;

    StronglyConnectedComponents(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("StronglyConnectedComponents", num_channels, spmv_out_buf_len, vec_buf_len) {}

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

    // labels of the padded matrix's vertices (padding vertices are singletons).  The priorities graphlily::io::
    // util_coloring_priorities gives for "natural", "random" or "largest_first" on degrees() decide which component every pass
    // removes -- its best-keyed live vertex's -- and never the labels: hubs first normally collects the giant component in pass
    // 1.  Leaves labels(), priorities() (empty for "natural"), passes(), trimmed(), rounds(), launches() and, over the real
    // vertices, num_components(), largest_component(), component_labels() (ascending), component_sizes() and is_dag().  The
    // call waits for the device.
    aligned_label_vec_t run(std::string order = "largest_first", uint32_t seed = 0) {
        require_sent("run()");
        if (order != "natural" && order != "random" && order != "largest_first") {
            printf("StronglyConnectedComponents::run(): order \"%s\" is none of natural, random, largest_first\n", order.c_str());
            exit(EXIT_FAILURE);
        }
        const size_t n = matrix_num_rows_;
        priorities_ = graphlily::io::util_coloring_priorities(degrees_, order, seed);
        const bool with_prio = !priorities_.empty();
        DeviceBuffer out(sizeof(uint32_t) * (with_prio ? 2 * n : n));       // the labels, then the priorities
        if (with_prio) GRAPHLILY_CHECK(gl_buf_h2d((uint32_t *)out.ptr() + n, priorities_.data(), sizeof(uint32_t) * n));
        uint64_t stats[5] = {0, 0, 0, 0, 0};
        SpMV_->scc(symmetric_ ? nullptr : out_, out, with_prio ? (const uint32_t *)out.ptr() + n : nullptr, stats);
        aligned_label_vec_t label(n);
        out.download(label.data(), sizeof(uint32_t) * n);
        labels_.assign(label.begin(), label.end());
        const uint64_t padding = n - n_real_;
        num_components_ = stats[0] - padding;
        passes_ = stats[1];
        trimmed_ = graph_.adj_indices.empty() ? 0 : stats[2] - padding;       // (every padding vertex was trimmed)
        rounds_ = stats[3];
        launches_ = stats[4];
        std::map<uint32_t, uint64_t> sizes;
        for (uint32_t v = 0; v < n_real_; v++) sizes[label[v]]++;
        component_labels_.clear();
        component_sizes_.clear();
        largest_component_ = 0;
        for (std::map<uint32_t, uint64_t>::const_iterator it = sizes.begin(); it != sizes.end(); ++it) {
            component_labels_.push_back(it->first);
            component_sizes_.push_back(it->second);
            largest_component_ = std::max(largest_component_, it->second);
        }
        return label;
    }
    const CSRMatrix<float> &graph() const { return graph_; }                    // row v: the predecessors of v
    const CSRMatrix<float> &graph_out() const { return symmetric_ ? graph_ : graph_out_; }      // row v: its successors
    bool symmetric() const { return symmetric_; }
    const std::vector<uint32_t> &labels() const { return labels_; }
    const std::vector<uint32_t> &priorities() const { return priorities_; }     // empty for "natural"
    uint64_t num_components() const { return num_components_; }                 // over the real vertices, as the next four
    uint64_t largest_component() const { return largest_component_; }
    const std::vector<uint32_t> &component_labels() const { return component_labels_; }     // ascending
    const std::vector<uint64_t> &component_sizes() const { return component_sizes_; }       // aligned with component_labels()
    bool is_dag() const { return largest_component_ <= 1; }                     // every component is a single vertex
    uint64_t passes() const { return passes_; }
    uint64_t trimmed() const { return trimmed_; }
    uint64_t rounds() const { return rounds_; }
    uint64_t launches() const { return launches_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_SCC_H_
