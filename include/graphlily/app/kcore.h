// graphlily/app/kcore.h -- k-core decomposition over the MI355X backend (an extension: the reference has no such driver), with
// the conventions of the drivers next to it (graphlily/app/tc.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_kcore peels
// (include/graphlily_hip.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and stored in both directions by the host
// (graphlily::io::util_symmetrize_simple): peeling v must reach every neighbour of v through row v.
//   core[v] = the largest k such that v lies in a subgraph in which every vertex has degree >= k
// Row shards are not supported: the kernel reads row u for every column u of a row.
#ifndef GRAPHLILY_HIP_APP_KCORE_H_
#define GRAPHLILY_HIP_APP_KCORE_H_

#include "graphlily/app/pattern_app.h"

#include <vector>

namespace graphlily {
namespace app {

class KCore : public app::PatternApp {
private:
    std::vector<uint32_t> order_;
    std::vector<uint64_t> core_sizes_;
    uint32_t degeneracy_ = 0, levels_ = 0, sub_rounds_ = 0, launches_ = 0;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        return graphlily::io::util_symmetrize_simple(padded, degrees_);
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_core_vec_t;

    KCore(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("KCore", num_channels, spmv_out_buf_len, vec_buf_len) {}

    // core numbers of the padded matrix's vertices (padding vertices: 0); leaves degeneracy(), levels(), sub_rounds(),
    // core_sizes() and, with want_order, order(): a degeneracy ordering (not unique).  The call waits for the device.
    aligned_core_vec_t run(bool want_order = false) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, words = want_order ? 2 * n : n;
        DeviceBuffer out(sizeof(uint32_t) * words);                  // the core numbers, then the order
        uint32_t stats[4] = {0, 0, 0, 0};
        SpMV_->kcore(out, want_order ? (uint32_t *)out.ptr() + n : nullptr, stats);
        aligned_core_vec_t core(words);
        out.download(core.data(), sizeof(uint32_t) * words);
        order_.assign(core.begin() + n, core.end());
        core.resize(n);
        degeneracy_ = stats[0];
        levels_ = stats[1];
        sub_rounds_ = stats[2];
        launches_ = stats[3];
        std::vector<uint64_t> count((size_t)degeneracy_ + 2, 0);
        for (uint32_t v = 0; v < n_real_; v++) count[core[v] <= degeneracy_ ? core[v] : degeneracy_ + 1]++;
        core_sizes_.assign((size_t)degeneracy_ + 1, 0);
        uint64_t above = count[(size_t)degeneracy_ + 1];
        for (size_t k = (size_t)degeneracy_ + 1; k-- > 0;) core_sizes_[k] = above += count[k];
        return core;
    }
    uint32_t degeneracy() const { return degeneracy_; }
    uint32_t levels() const { return levels_; }
    uint32_t sub_rounds() const { return sub_rounds_; }
    uint32_t launches() const { return launches_; }
    const std::vector<uint32_t> &order() const { return order_; }               // empty unless run(true)
    const std::vector<uint64_t> &core_sizes() const { return core_sizes_; }     // [k] = real vertices with core >= k
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_KCORE_H_
