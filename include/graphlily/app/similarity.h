// graphlily/app/similarity.h -- neighbourhood similarity and link prediction over the MI355X backend (an extension: the reference
// has no such driver), with the conventions of the drivers next to it (graphlily/app/kcore.h): print and exit on error,
// device-resident buffers.  One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row
// copy gl_similarity intersects (include/graphlily_hip_sim.h).  The matrix is read as an undirected simple graph
// (graphlily::io::util_symmetrize_simple), as KCore reads it.  For caller-chosen pairs (u, v) -- which need not be edges -- with
// c = |N(u) & N(v)| and the degrees du, dv, all in f64 on the host from the kernel's integers, 0.0 where a denominator is 0:
//   jaccard = c / (du + dv - c), overlap = c / min(du, dv), sorensen = 2 c / (du + dv), cosine = c / sqrt(du dv),
//   preferential_attachment = du dv (no kernel), adamic_adar = sum of 1 / ln(deg w), resource_allocation = sum of 1 / deg w over
//   the common neighbours w.
// The two weighted measures travel as FIXED POINT: shift = 62 - bit_length(max degree), aa[w] = round(2^shift / ln(deg w)), ra[w] =
// round(2^shift / deg w) where deg w >= 2, else 0; a sum over at most max degree terms below 2^(shift + 1) stays below 2^63, so
// the kernel's 64-bit integer sums never wrap here, and integer adds give the same bits whatever the order.
// Row shards are not supported: the kernel reads the rows of both vertices of a pair.
#ifndef GRAPHLILY_HIP_APP_SIMILARITY_H_
#define GRAPHLILY_HIP_APP_SIMILARITY_H_

#include "graphlily/app/pattern_app.h"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace graphlily {
namespace app {

class Similarity : public app::PatternApp {
public:
    enum Measure { kCommon = 0, kJaccard, kOverlap, kSorensen, kCosine, kPreferentialAttachment, kAdamicAdar, kResourceAllocation };
    typedef std::vector<std::pair<uint32_t, uint32_t>> pairs_t;

private:
    CSRMatrix<float> graph_;
    std::vector<uint64_t> aa_, ra_, weighted_[2];      // weighted_[0]: the Adamic-Adar sums of the last run, [1]: resource allocation
    std::vector<uint32_t> common_;
    pairs_t pairs_, edges_;
    DeviceBuffer aa_buf_, ra_buf_;
    int shift_ = 62;
    uint64_t launches_ = 0, deferred_ = 0;

    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        graph_ = graphlily::io::util_symmetrize_simple(padded, degrees_);
        uint32_t most = 0;
        for (uint32_t d : degrees_) most = std::max(most, d);
        int bits = 0;
        for (uint32_t x = most; x; x >>= 1) bits++;
        shift_ = 62 - bits;
        const double one = std::ldexp(1.0, shift_);
        aa_.assign(degrees_.size(), 0);
        ra_.assign(degrees_.size(), 0);
        for (size_t w = 0; w < degrees_.size(); w++) {
            if (degrees_[w] < 2) continue;
            aa_[w] = (uint64_t)std::nearbyint(one / std::log((double)degrees_[w]));
            ra_[w] = (uint64_t)std::nearbyint(one / (double)degrees_[w]);
        }
        return graph_;
    }

public:
    Similarity(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("Similarity", num_channels, spmv_out_buf_len, vec_buf_len) {}

    // ... and the two fixed-point weight tables, num_vertices() 64-bit words each
    void send_matrix_host_to_device() {
        PatternApp::send_matrix_host_to_device();
        const size_t n = aa_.size();
        aa_buf_ = DeviceBuffer(sizeof(uint64_t) * (n ? n : 1));
        ra_buf_ = DeviceBuffer(sizeof(uint64_t) * (n ? n : 1));
        if (n) {
            aa_buf_.upload(aa_.data(), sizeof(uint64_t) * n);
            ra_buf_.upload(ra_.data(), sizeof(uint64_t) * n);
        }
    }

    // the common neighbours of every pair (real vertices; u == v is legal), and with want_adamic_adar / want_resource_allocation the
    // fixed-point sums: gl_similarity once per table asked for, once without a table when neither is.  Leaves common(), pairs(),
    // adamic_adar_sums(), resource_allocation_sums(), deferred() and launches(); score() gives the measures.  Waits for the device.
    const std::vector<uint32_t> &run(const pairs_t &pairs, bool want_adamic_adar = false, bool want_resource_allocation = false) {
        require_sent("run()");
        const size_t m = pairs.size();
        if (m > 0xffffffffull) {
            printf("%s::run(): %zu pairs, at most 2^32 - 1 per call\n", name_, m);
            exit(EXIT_FAILURE);
        }
        std::vector<uint32_t> flat(2 * m);
        for (size_t i = 0; i < m; i++) {
            if (pairs[i].first >= n_real_ || pairs[i].second >= n_real_) {
                printf("%s::run(): pair %zu = (%u, %u) names no real vertex\n", name_, i, pairs[i].first, pairs[i].second);
                exit(EXIT_FAILURE);
            }
            flat[2 * i] = pairs[i].first;
            flat[2 * i + 1] = pairs[i].second;
        }
        pairs_ = pairs;
        launches_ = deferred_ = 0;
        common_.assign(m, 0);
        weighted_[0].assign(want_adamic_adar ? m : 0, 0);
        weighted_[1].assign(want_resource_allocation ? m : 0, 0);
        if (!m) return common_;
        DeviceBuffer pairs_buf(sizeof(uint32_t) * 2 * m), common_buf(sizeof(uint32_t) * m), weighted_buf(sizeof(uint64_t) * m);
        pairs_buf.upload(flat.data(), sizeof(uint32_t) * 2 * m);
        const bool want[2] = {want_adamic_adar, want_resource_allocation};
        const DeviceBuffer *table[2] = {&aa_buf_, &ra_buf_};
        const bool plain = !want[0] && !want[1];
        for (int t = 0; t < 2; t++) {
            if (!want[t] && !(plain && t == 0)) continue;
            uint64_t stats[4] = {0, 0, 0, 0};
            SpMV_->similarity((const uint32_t *)pairs_buf.ptr(), m, (uint32_t *)common_buf.ptr(),
                              plain ? nullptr : (uint64_t *)weighted_buf.ptr(), plain ? nullptr : (const uint64_t *)table[t]->ptr(), stats);
            deferred_ = stats[1];
            launches_ += stats[2];
            if (!plain) weighted_buf.download(weighted_[t].data(), sizeof(uint64_t) * m);
        }
        common_buf.download(common_.data(), sizeof(uint32_t) * m);
        return common_;
    }

    // run() over every edge {u, v}, u < v, of the prepared graph, ascending; leaves edges()
    const std::vector<uint32_t> &run_edges(bool want_adamic_adar = false, bool want_resource_allocation = false) {
        require_sent("run_edges()");
        edges_.clear();
        for (size_t v = 0; v < matrix_num_rows_; v++)
            for (uint32_t j = graph_.adj_indptr[v]; j < graph_.adj_indptr[v + 1]; j++)
                if (graph_.adj_indices[j] > v) edges_.push_back(std::make_pair((uint32_t)v, graph_.adj_indices[j]));
        return run(edges_, want_adamic_adar, want_resource_allocation);
    }

    // one measure of the last run, aligned with pairs(): f64 from the integers (common and preferential_attachment are exact
    // integers below 2^53 -- below 2^64 -- as doubles); the weighted ones need the run to have asked for their table
    std::vector<double> score(Measure measure) const {
        const size_t m = pairs_.size();
        std::vector<double> out(m, 0.0);
        if ((measure == kAdamicAdar && weighted_[0].size() != m) || (measure == kResourceAllocation && weighted_[1].size() != m)) {
            printf("%s::score(): the last run() did not ask for this weighted measure\n", name_);
            exit(EXIT_FAILURE);
        }
        for (size_t i = 0; i < m; i++) {
            const double c = (double)common_[i], du = (double)degrees_[pairs_[i].first], dv = (double)degrees_[pairs_[i].second];
            double num = c, den = 1.0;
            switch (measure) {
                case kCommon: break;
                case kJaccard: den = du + dv - c; break;
                case kOverlap: den = std::min(du, dv); break;
                case kSorensen: num = 2.0 * c; den = du + dv; break;
                case kCosine: den = std::sqrt(du * dv); break;
                case kPreferentialAttachment: num = (double)((uint64_t)degrees_[pairs_[i].first] * (uint64_t)degrees_[pairs_[i].second]); break;
                case kAdamicAdar: num = (double)weighted_[0][i] * std::ldexp(1.0, -shift_); break;
                case kResourceAllocation: num = (double)weighted_[1][i] * std::ldexp(1.0, -shift_); break;
            }
            out[i] = den > 0 ? num / den : 0.0;
        }
        return out;
    }

    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric matrix: row v lists the neighbours of v
    int shift() const { return shift_; }
    const std::vector<uint64_t> &adamic_adar_weights() const { return aa_; }
    const std::vector<uint64_t> &resource_allocation_weights() const { return ra_; }
    const std::vector<uint32_t> &common() const { return common_; }
    const std::vector<uint64_t> &adamic_adar_sums() const { return weighted_[0]; }              // fixed point at shift()
    const std::vector<uint64_t> &resource_allocation_sums() const { return weighted_[1]; }
    const pairs_t &pairs() const { return pairs_; }
    const pairs_t &edges() const { return edges_; }
    uint64_t launches() const { return launches_; }
    uint64_t deferred() const { return deferred_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_SIMILARITY_H_
