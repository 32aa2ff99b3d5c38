// graphlily/app/lpa.h -- label propagation communities over the MI355X backend (an extension: the reference has no such driver),
// with the conventions of the drivers next to it (graphlily/app/coloring.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_lpa walks
// (include/graphlily_hip_lpa.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and stored in both directions by the host
// (graphlily::io::util_symmetrize_simple).
//   evaluating v: cnt(l) = neighbours carrying l; if max cnt > cnt(label[v]), label[v] becomes the smallest l with cnt(l) == max cnt
//   a sweep evaluates colour class 0, then class 1, ... in place under a proper colouring (gl_color's, on the same plan): the
//   sequential loop in (colour, vertex) order, which reaches a fixed point; synchronous = true sweeps all vertices at once
// Row shards are not supported: the kernel reads the label of every column of a row.
#ifndef GRAPHLILY_HIP_APP_LPA_H_
#define GRAPHLILY_HIP_APP_LPA_H_

#include "graphlily/app/pattern_app.h"

#include <algorithm>
#include <string>
#include <vector>

namespace graphlily {
namespace app {

class LabelPropagation : public app::PatternApp {
private:
    CSRMatrix<float> graph_;
    std::vector<uint32_t> labels_, colors_, initial_, community_labels_;
    std::vector<uint64_t> community_sizes_;
    uint64_t num_colors_ = 0, sweeps_ = 0, changes_ = 0, evaluations_ = 0, launches_ = 0, converged_ = 0;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        graph_ = graphlily::io::util_symmetrize_simple(padded, degrees_);
        return graph_;
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_label_vec_t;

    LabelPropagation(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("LabelPropagation", num_channels, spmv_out_buf_len, vec_buf_len) {}

    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric matrix

    // labels of the padded matrix's vertices (padding vertices keep their own numbers), swept under the colouring gl_color gives
    // on the same plan for graphlily::io::util_coloring_priorities(degrees(), order, seed) ("smallest_last" first runs gl_kcore),
    // or synchronously; with_seed: the vertices start with graphlily::io::util_lpa_initial_labels(num_real_vertices(), seed), a
    // permutation, otherwise with their own numbers; `initial` (num_real_vertices() or num_vertices() words), if not empty,
    // overrides both.  Leaves labels(), colors() (empty when synchronous), num_colors(), initial() (empty for own numbers),
    // sweeps(), changes(), evaluations(), launches(), converged(), num_communities(), community_labels(), community_sizes() and
    // modularity().  The call waits for the device.
    aligned_label_vec_t run(uint32_t max_sweeps = 100, std::string order = "largest_first", bool with_seed = false, uint32_t seed = 0,
                            bool synchronous = false, std::vector<uint32_t> const &initial = std::vector<uint32_t>()) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, words = n ? n : 1;
        DeviceBuffer out(sizeof(uint32_t) * words), color(sizeof(uint32_t) * words), third(sizeof(uint32_t) * words);   // third: the priorities, then the initial labels
        uint32_t *d_color = (uint32_t *)color.ptr(), *d_third = (uint32_t *)third.ptr();
        initial_.clear();
        if (!initial.empty()) {
            if (initial.size() != n_real_ && initial.size() != n) {
                printf("LabelPropagation::run(): %zu initial labels, expected %u or %zu\n", initial.size(), n_real_, n);
                exit(EXIT_FAILURE);
            }
            initial_ = initial;
            for (size_t v = initial.size(); v < n; v++) initial_.push_back((uint32_t)v);
        } else if (with_seed) {
            initial_ = graphlily::io::util_lpa_initial_labels(n_real_, seed, (uint32_t)n);
        }
        colors_.clear();
        num_colors_ = 1;
        if (!synchronous) {
            const uint32_t seed0 = with_seed ? seed : 0;
            std::vector<uint32_t> prio;
            if (order == "smallest_last")
                prio = graphlily::io::util_coloring_priorities(degrees_, order, seed0, peel_order());
            else
                prio = graphlily::io::util_coloring_priorities(degrees_, order, seed0);
            if (!prio.empty()) GRAPHLILY_CHECK(gl_buf_h2d(d_third, prio.data(), sizeof(uint32_t) * n));
            uint64_t cstats[4] = {0, 0, 0, 0};
            SpMV_->color(color, prio.empty() ? nullptr : d_third, cstats);
            num_colors_ = cstats[0];
        }
        if (!initial_.empty()) GRAPHLILY_CHECK(gl_buf_h2d(d_third, initial_.data(), sizeof(uint32_t) * n));
        uint64_t stats[5] = {0, 0, 0, 0, 0};
        SpMV_->lpa(out, synchronous ? nullptr : d_color, initial_.empty() ? nullptr : d_third, max_sweeps, stats);
        aligned_label_vec_t label(words);
        out.download(label.data(), sizeof(uint32_t) * words);
        label.resize(n);
        labels_.assign(label.begin(), label.end());
        if (!synchronous) {
            colors_.assign(words, 0);
            color.download(colors_.data(), sizeof(uint32_t) * words);
            colors_.resize(n);
        }
        sweeps_ = stats[0];
        changes_ = stats[1];
        evaluations_ = stats[2];
        launches_ = stats[3];
        converged_ = stats[4];
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
        return label;
    }
    const std::vector<uint32_t> &labels() const { return labels_; }                 // the last run()'s result
    const std::vector<uint32_t> &colors() const { return colors_; }                 // the colouring it swept by (empty: synchronous)
    const std::vector<uint32_t> &initial() const { return initial_; }               // the labels it started from (empty: own numbers)
    uint64_t num_colors() const { return num_colors_; }
    uint64_t sweeps() const { return sweeps_; }
    uint64_t changes() const { return changes_; }
    uint64_t evaluations() const { return evaluations_; }
    uint64_t launches() const { return launches_; }                                  // gl_lpa's alone
    bool converged() const { return converged_ != 0; }
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

#endif  // GRAPHLILY_HIP_APP_LPA_H_
