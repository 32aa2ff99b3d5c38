// graphlily/app/cc.h -- weakly connected components over the MI355X backend (an extension: the reference has no such driver),
// with the conventions of the three drivers next to it (graphlily/app/bfs.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_cc_labels walks
// (include/graphlily_hip.h): lock-free union-find over the rows, then pointer doubling.
//   labels[v] = the smallest vertex joined to v by a chain of stored entries, taken in either direction
// Row shards are not supported: every rank would hold the forest of its own rows and the forests would have to be merged.  On
// one device gl_cc_hook composes: gl_cc_begin, gl_cc_hook on every shard's plan, gl_cc_finish.
#ifndef GRAPHLILY_HIP_APP_CC_H_
#define GRAPHLILY_HIP_APP_CC_H_

#include "graphlily/app/pattern_app.h"

#include <algorithm>
#include <vector>

namespace graphlily {
namespace app {

class ConnectedComponents : public app::PatternApp {
private:
    uint32_t num_components_ = 0, largest_component_ = 0;

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_label_vec_t;

    ConnectedComponents(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("ConnectedComponents", num_channels, spmv_out_buf_len, vec_buf_len) {}      // (PatternApp's prepare(): every stored entry an edge)

    // labels of the padded matrix's vertices (padding vertices are singletons); leaves num_components() -- over the real
    // vertices -- and largest_component()
    aligned_label_vec_t run() {
        require_sent("run()");
        const uint32_t n = matrix_num_rows_;
        DeviceBuffer out(sizeof(uint32_t) * ((size_t)n + 1));      // vertex numbers, then the component count
        SpMV_->cc_labels(out, (uint32_t *)out.ptr() + n);
        aligned_label_vec_t labels((size_t)n + 1);
        out.download(labels.data(), sizeof(uint32_t) * ((size_t)n + 1));
        num_components_ = labels[n] - (n - n_real_);
        labels.resize(n);
        std::vector<uint32_t> size(n, 0);
        largest_component_ = 0;
        for (uint32_t v = 0; v < n; v++)
            if (labels[v] < n) largest_component_ = std::max(largest_component_, ++size[labels[v]]);
        return labels;
    }
    uint32_t num_components() const { return num_components_; }
    uint32_t largest_component() const { return largest_component_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_CC_H_
