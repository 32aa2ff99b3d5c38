// graphlily/app/topo.h -- topological levels, a topological order and the critical path over the MI355X backend (an extension: the
// reference has no such driver), with the conventions of the drivers next to it (graphlily/app/scc.h): print and exit on error,
// device-resident buffers.  The matrix is read as a DIRECTED graph (graphlily::io::util_directed_weighted: an edge u -> v for a
// stored entry A[v,u], u != v; weighted = false is util_simple_pattern's reading, weighted = true keeps every stored entry with
// the largest of its values, -0.0 as +0.0, NaN and inf refused).  One SpMVModule with the (||,&&) semiring holds the pattern, so
// that the plan is the boolean layout, whose plain row copy gl_topo walks (include/graphlily_hip_topo.h); a second
// one holds the transposed pattern and is loaded only when the pattern is not symmetric, as in graphlily/app/scc.h.  Both plans are
// built from ones; the weights travel in buffers of their own, aligned with graph().adj_indices and graph_out().adj_indices.
//   level[v]  = the edges of the longest path that ends in v; 0xffffffff on a cycle or behind one
//   dist[v]   = the largest f32 dist[u] + w(u, v) over the predecessors, +0 on a source; parent[v] = the smallest u that attains it
// Row shards are not supported: the kernel decrements the counter of every column of a row of the transposed pattern.
#ifndef GRAPHLILY_HIP_APP_TOPO_H_
#define GRAPHLILY_HIP_APP_TOPO_H_

#include "graphlily/app/pattern_app.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace graphlily {
namespace app {

class TopologicalOrder : public app::PatternApp {
private:
    // the transposed pattern's module: created by the first load that needs two plans (owned by the collection from then on)
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *out_ = nullptr;
    CSRMatrix<float> graph_, graph_out_;
    DeviceBuffer weight_, weight_out_;
    bool runtime_up_ = false, symmetric_ = true, weighted_ = false;
    std::vector<uint32_t> level_, parent_, order_, position_;
    std::vector<float> dist_;
    std::vector<uint64_t> level_sizes_;
    uint64_t num_peeled_ = 0, widest_ = 0, launches_ = 0;
    float critical_length_ = 0.0f;

    static CSRMatrix<float> ones_of(CSRMatrix<float> const &g) {
        CSRMatrix<float> ones = g;
        ones.adj_data.assign(ones.adj_indices.size(), 1.0f);
        return ones;
    }

    // get_nnz() counts the edges of the directed graph
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        symmetric_ = graphlily::io::util_directed_weighted(padded, graph_, graph_out_, weighted_);
        return ones_of(graph_);
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_level_vec_t;

    TopologicalOrder(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("TopologicalOrder", num_channels, spmv_out_buf_len, vec_buf_len) {}

    void set_up_runtime(std::string xclbin_file_path) {
        ModuleCollection::set_up_runtime(xclbin_file_path);
        runtime_up_ = true;
    }

    void load_and_format_matrix(std::string csr_float_npz_path, bool skip_empty_rows, bool weighted = false) {
        weighted_ = weighted;
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
        out_->load_and_format_matrix(ones_of(graph_out_), skip_empty_rows);
    }

    void send_matrix_host_to_device() {
        PatternApp::send_matrix_host_to_device();
        if (!symmetric_) out_->send_matrix_host_to_device();
        if (!weighted_) return;
        const size_t nnz = graph_.adj_data.size();
        weight_ = DeviceBuffer(sizeof(float) * (nnz ? nnz : 1));
        weight_out_ = DeviceBuffer(sizeof(float) * (nnz ? nnz : 1));
        if (nnz) {
            weight_.upload(graph_.adj_data.data(), sizeof(float) * nnz);
            weight_out_.upload(graph_out_.adj_data.data(), sizeof(float) * nnz);
        }
    }

    // levels of the padded matrix's vertices (padding vertices are isolated: level 0); reverse swaps the two plans: heights, and
    // the distance to a sink.  Leaves level(), launches() and, over the real vertices, num_peeled(), is_dag(), level_sizes(),
    // num_levels() and widest(); on a weighted load dist(), parent() and critical_length(); with want_order order() -- the peeled
    // real vertices sorted by (level, vertex), canonicalised on the host from the device's queue -- and position().  The call
    // waits for the device.
    aligned_level_vec_t run(bool reverse = false, bool want_order = false) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, room = n ? n : 1;
        DeviceBuffer out(sizeof(uint32_t) * 4 * room);              // level, queue, dist, parent
        uint32_t *words = (uint32_t *)out.ptr();
        uint64_t stats[4] = {0, 0, 0, 0};
        graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *pin = SpMV_, *pout = symmetric_ ? nullptr : out_;
        if (reverse && !symmetric_) std::swap(pin, pout);
        const float *w = weighted_ ? (const float *)(reverse ? weight_out_ : weight_).ptr() : nullptr;
        pin->topo(pout, out, want_order ? words + room : nullptr, w, weighted_ ? (float *)(words + 2 * room) : nullptr,
                  weighted_ ? words + 3 * room : nullptr, stats);
        aligned_level_vec_t got(4 * room);
        out.download(got.data(), sizeof(uint32_t) * 4 * room);
        level_.assign(got.begin(), got.begin() + n);
        level_sizes_.clear();
        num_peeled_ = 0;
        for (uint32_t v = 0; v < n_real_; v++) {
            if (level_[v] == 0xffffffffu) continue;
            num_peeled_++;
            if (level_[v] >= level_sizes_.size()) level_sizes_.resize((size_t)level_[v] + 1, 0);
            level_sizes_[level_[v]]++;
        }
        widest_ = 0;
        for (uint64_t c : level_sizes_) widest_ = std::max(widest_, c);
        launches_ = stats[3];
        dist_.clear();
        parent_.clear();
        critical_length_ = 0.0f;
        if (weighted_) {
            dist_.resize(n);
            memcpy(dist_.data(), got.data() + 2 * room, sizeof(float) * n);
            parent_.assign(got.begin() + 3 * room, got.begin() + 3 * room + n);
            bool any = false;
            for (uint32_t v = 0; v < n_real_; v++)
                if (level_[v] != 0xffffffffu && (!any || dist_[v] > critical_length_)) {
                    critical_length_ = dist_[v];
                    any = true;
                }
        }
        order_.clear();
        position_.clear();
        if (want_order) {
            std::vector<std::pair<uint32_t, uint32_t>> key;         // (level, vertex)
            for (size_t i = 0; i < stats[0]; i++) {
                const uint32_t v = got[room + i];
                if (v < n_real_) key.push_back(std::make_pair(level_[v], v));
            }
            std::sort(key.begin(), key.end());
            position_.assign(n_real_, 0xffffffffu);
            for (size_t i = 0; i < key.size(); i++) {
                order_.push_back(key[i].second);
                position_[key[i].second] = (uint32_t)i;
            }
        }
        return aligned_level_vec_t(got.begin(), got.begin() + n);
    }

    // the vertices of a longest weighted path of the last run: from the smallest real vertex of largest dist() back along parent()
    std::vector<uint32_t> critical_path() const {
        std::vector<uint32_t> path;
        if (dist_.empty() || !num_peeled_) return path;
        for (uint32_t v = 0; v < n_real_ && path.empty(); v++)
            if (level_[v] != 0xffffffffu && dist_[v] == critical_length_) path.push_back(v);
        while (parent_[path.back()] != 0xffffffffu) path.push_back(parent_[path.back()]);
        return path;
    }

    const CSRMatrix<float> &graph() const { return graph_; }                    // row v: the predecessors of v (weights in adj_data)
    const CSRMatrix<float> &graph_out() const { return symmetric_ && !weighted_ ? graph_ : graph_out_; }      // row v: its successors
    bool symmetric() const { return symmetric_; }
    const std::vector<uint32_t> &level() const { return level_; }
    const std::vector<float> &dist() const { return dist_; }                    // empty unless the load was weighted
    const std::vector<uint32_t> &parent() const { return parent_; }
    const std::vector<uint32_t> &order() const { return order_; }               // empty unless run(.., true)
    const std::vector<uint32_t> &position() const { return position_; }
    uint64_t num_peeled() const { return num_peeled_; }                         // over the real vertices, as the next four
    bool is_dag() const { return num_peeled_ == n_real_; }
    const std::vector<uint64_t> &level_sizes() const { return level_sizes_; }
    uint64_t num_levels() const { return level_sizes_.size(); }
    uint64_t widest() const { return widest_; }
    float critical_length() const { return critical_length_; }
    uint64_t launches() const { return launches_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_TOPO_H_
