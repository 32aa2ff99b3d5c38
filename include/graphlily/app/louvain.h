// graphlily/app/louvain.h -- Louvain communities over the MI355X backend (an extension: the reference has no such driver), with
// the conventions of the drivers next to it (graphlily/app/lpa.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_louvain_move walks
// (include/graphlily_hip_louvain.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored; input weights are not read -- and stored in both directions by the host
// (graphlily::io::util_symmetrize_simple).
//   a level: colour the level's pattern (gl_color on its plan), move the vertices class by class until a sweep gains no more than
//   tol (gl_louvain_move, integers throughout), aggregate the communities on the host (graphlily::io::util_aggregate_communities)
//   into the next level's weighted graph, which gets a fresh SpMVModule plan
// Row shards are not supported: the kernel reads the label of every column of a row and the whole tot array.
#ifndef GRAPHLILY_HIP_APP_LOUVAIN_H_
#define GRAPHLILY_HIP_APP_LOUVAIN_H_

#include "graphlily/app/pattern_app.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

namespace graphlily {
namespace app {

class Louvain : public app::PatternApp {
private:
    typedef graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> spmv_t;
    CSRMatrix<float> graph_;
    std::vector<uint32_t> labels_, community_labels_;
    std::vector<uint64_t> community_sizes_, level_sizes_, level_colors_, level_sweeps_, level_moves_;
    std::vector<std::pair<int64_t, int64_t>> level_q_;
    std::vector<std::vector<uint32_t>> dendrogram_;
    uint64_t levels_ = 0, launches_ = 0;
    bool runtime_up_ = false;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        graph_ = graphlily::io::util_symmetrize_simple(padded, degrees_);
        return graph_;
    }

    // a level's own module: the aggregated pattern, padded as the driver pads its matrix
    spmv_t *module_of(CSRMatrix<float> padded) {
        graphlily::io::util_round_csr_matrix_dim(padded, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        spmv_t *mod = new spmv_t(num_channels_, spmv_out_buf_len_, vec_buf_len_);
        mod->set_semiring(graphlily::LogicalSemiring);
        mod->set_mask_type(graphlily::kNoMask);
        if (runtime_up_) {      // what ModuleCollection::set_up_runtime does per module
            mod->set_device(device_);
            mod->set_unused_args();
            mod->set_mode();
            mod->set_blocking(getenv("GRAPHLILY_BLOCKING") != nullptr && atoi(getenv("GRAPHLILY_BLOCKING")) != 0);
        }
        mod->load_and_format_matrix(padded, true);
        mod->send_matrix_host_to_device();
        return mod;
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_label_vec_t;

    Louvain(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("Louvain", num_channels, spmv_out_buf_len, vec_buf_len) {}

    void set_up_runtime(std::string xclbin_file_path) {
        ModuleCollection::set_up_runtime(xclbin_file_path);
        runtime_up_ = true;
    }

    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric matrix

    // labels of the padded matrix's vertices: every vertex carries the SMALLEST original vertex of its community (isolated and
    // padding vertices keep their own numbers).  Level 0 runs on this driver's own module, every later level on a fresh plan of
    // the aggregated pattern; each level is coloured by gl_color under graphlily::io::util_coloring_priorities(that level's pattern
    // degrees, order, seed) ("smallest_last" first runs gl_kcore on the level's plan) and moved with min_gain = floor(tol * two_m^2).
    // A level is ACCEPTED iff it moved something and its q_last is strictly above the last accepted Q (at the start: the singletons'
    // Q); otherwise it is discarded and the run ends, as it does when a level merges nothing or max_levels is reached.  Leaves
    // labels(), levels() (accepted), per level RUN (a discarded last one included) level_sizes(), level_colors(), level_sweeps(),
    // level_moves() and level_q() (q_first, q_last: modularity x two_m^2), launches(), dendrogram(), num_communities(),
    // community_labels(), community_sizes() and modularity().  The call waits for the device.
    aligned_label_vec_t run(double tol = 1e-7, uint32_t max_sweeps = 100, uint32_t max_levels = 32, std::string order = "largest_first",
                            uint32_t seed = 0) {
        require_sent("run()");
        const size_t n = matrix_num_rows_;
        CSRMatrix<float> graph = graph_;
        std::vector<uint32_t> weights, k(degrees_), community_of(n);
        for (size_t v = 0; v < n; v++) community_of[v] = (uint32_t)v;
        level_sizes_.clear();
        level_colors_.clear();
        level_sweeps_.clear();
        level_moves_.clear();
        level_q_.clear();
        dendrogram_.clear();
        levels_ = launches_ = 0;
        int64_t accepted = 0;
        for (uint32_t level = 0; level < max_levels; level++) {
            spmv_t *mod = level == 0 ? SpMV_ : module_of(graph);
            const size_t rows = mod->get_num_rows(), words = rows ? rows : 1, nnz = graph.adj_indices.size();
            std::vector<uint32_t> deg(rows, 0);
            for (size_t v = 0; v < graph.num_rows; v++) deg[v] = graph.adj_indptr[v + 1] - graph.adj_indptr[v];
            DeviceBuffer label(sizeof(uint32_t) * words), color(sizeof(uint32_t) * words), third(sizeof(uint32_t) * words);
            DeviceBuffer weight(sizeof(uint32_t) * (nnz ? nnz : 1));
            std::vector<uint32_t> prio;
            if (order == "smallest_last") {
                DeviceBuffer peel(sizeof(uint32_t) * 2 * words);
                mod->kcore(peel, (uint32_t *)peel.ptr() + rows);
                std::vector<uint32_t> both(2 * words);
                peel.download(both.data(), sizeof(uint32_t) * 2 * rows);
                prio = graphlily::io::util_coloring_priorities(deg, order, seed, std::vector<uint32_t>(both.begin() + rows, both.begin() + 2 * rows));
            } else {
                prio = graphlily::io::util_coloring_priorities(deg, order, seed);
            }
            if (!prio.empty()) GRAPHLILY_CHECK(gl_buf_h2d(third.ptr(), prio.data(), sizeof(uint32_t) * rows));
            uint64_t cstats[4] = {0, 0, 0, 0};
            mod->color(color, prio.empty() ? nullptr : (const uint32_t *)third.ptr(), cstats);
            uint64_t two_m = 0;
            for (uint32_t x : k) two_m += x;
            const uint64_t min_gain = (uint64_t)std::floor(tol * (double)(two_m * two_m));
            if (level) {
                std::vector<uint32_t> kp(k);
                kp.resize(words, 0);
                GRAPHLILY_CHECK(gl_buf_h2d(third.ptr(), kp.data(), sizeof(uint32_t) * rows));
                if (nnz) GRAPHLILY_CHECK(gl_buf_h2d(weight.ptr(), weights.data(), sizeof(uint32_t) * nnz));
            }
            uint64_t stats[7] = {0, 0, 0, 0, 0, 0, 0};
            mod->louvain_move(label, (const uint32_t *)color.ptr(), level && nnz ? (const uint32_t *)weight.ptr() : nullptr,
                              level ? (const uint32_t *)third.ptr() : nullptr, max_sweeps, min_gain, stats);
            std::vector<uint32_t> lab(words);
            label.download(lab.data(), sizeof(uint32_t) * words);
            lab.resize(graph.num_rows);
            if (level) delete mod;
            const int64_t q_first = (int64_t)stats[5], q_last = (int64_t)stats[6];
            level_sizes_.push_back(graph.num_rows);
            level_colors_.push_back(cstats[0]);
            level_sweeps_.push_back(stats[0]);
            level_moves_.push_back(stats[1]);
            level_q_.push_back(std::make_pair(q_first, q_last));
            launches_ += stats[3];
            if (level == 0) accepted = q_first;
            if (stats[1] == 0 || q_last <= accepted) break;
            accepted = q_last;
            std::vector<uint32_t> next_weights, next_k, part;
            CSRMatrix<float> smaller = graphlily::io::util_aggregate_communities(graph, weights, k, lab, next_weights, next_k, part);
            for (size_t v = 0; v < n; v++) community_of[v] = part[community_of[v]];
            dendrogram_.push_back(community_of);
            levels_++;
            const bool merged = smaller.num_rows != graph.num_rows;
            graph = smaller;
            weights.swap(next_weights);
            k.swap(next_k);
            if (!merged) break;
        }
        std::vector<uint32_t> smallest(n, (uint32_t)n);
        for (size_t v = n; v-- > 0;) smallest[community_of[v]] = (uint32_t)v;
        aligned_label_vec_t out(n);
        for (size_t v = 0; v < n; v++) out[v] = smallest[community_of[v]];
        labels_.assign(out.begin(), out.end());
        std::vector<uint32_t> sorted(labels_.begin(), labels_.begin() + n_real_);
        std::sort(sorted.begin(), sorted.end());
        community_labels_.clear();
        community_sizes_.clear();
        for (size_t i = 0; i < sorted.size(); i++) {
            if (i == 0 || sorted[i] != sorted[i - 1]) {
                community_labels_.push_back(sorted[i]);
                community_sizes_.push_back(0);
            }
            community_sizes_.back()++;
        }
        return out;
    }
    const std::vector<uint32_t> &labels() const { return labels_; }                 // the last run()'s result
    uint64_t levels() const { return levels_; }                                      // accepted levels
    const std::vector<uint64_t> &level_sizes() const { return level_sizes_; }        // per level run: its vertices
    const std::vector<uint64_t> &level_colors() const { return level_colors_; }      // ... the classes swept
    const std::vector<uint64_t> &level_sweeps() const { return level_sweeps_; }
    const std::vector<uint64_t> &level_moves() const { return level_moves_; }
    const std::vector<std::pair<int64_t, int64_t>> &level_q() const { return level_q_; }     // (q_first, q_last)
    const std::vector<std::vector<uint32_t>> &dendrogram() const { return dendrogram_; }     // per accepted level
    uint64_t launches() const { return launches_; }                                  // gl_louvain_move's alone
    uint64_t num_communities() const { return community_labels_.size(); }            // over the real vertices
    const std::vector<uint32_t> &community_labels() const { return community_labels_; }    // ascending
    const std::vector<uint64_t> &community_sizes() const { return community_sizes_; }      // aligned with community_labels()

    // Newman's modularity sum_c e_c / m - (d_c / 2 m)^2 of the last run's labels on graph(), in f64 on the host (0 without edges)
    double modularity() const {
        const size_t n = labels_.size(), nnz = graph_.adj_indices.size();
        if (nnz == 0 || n == 0) return 0.0;
        std::vector<uint32_t> sorted(labels_);
        std::sort(sorted.begin(), sorted.end());
        sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
        std::vector<double> inside(sorted.size(), 0.0), degree(sorted.size(), 0.0);
        for (size_t v = 0; v < n; v++) {
            const size_t c = std::lower_bound(sorted.begin(), sorted.end(), labels_[v]) - sorted.begin();
            degree[c] += (double)degrees_[v];
            for (uint32_t j = graph_.adj_indptr[v]; j < graph_.adj_indptr[v + 1]; j++)
                if (labels_[graph_.adj_indices[j]] == labels_[v]) inside[c] += 1.0;      // (twice e_c)
        }
        double q = 0.0;
        for (size_t c = 0; c < sorted.size(); c++) q += inside[c] / (double)nnz - (degree[c] / (double)nnz) * (degree[c] / (double)nnz);
        return q;
    }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_LOUVAIN_H_
