// graphlily/app/bicc.h -- biconnected components over the MI355X backend (an extension: the reference has no such driver), with
// the conventions of the drivers next to it (graphlily/app/truss.h): print and exit on error, device-resident buffers.
// One SpMVModule with the (||,&&) semiring, so that the plan is the boolean layout, whose plain row copy gl_bicc walks
// (include/graphlily_hip_bicc.h).  The matrix is read as an undirected simple graph -- duplicates, the diagonal,
// zero-valued entries and direction are ignored -- and stored in both directions by the host
// (graphlily::io::util_symmetrize_simple); that matrix is kept as graph(), and blocks() has one word per ENTRY of it, aligned
// with graph().adj_indices: both entries of an edge carry the same value.
//   block[j]          = the smallest entry number of the block (biconnected component) that holds the edge of entry j
//   vertex_blocks[v]  = the blocks v belongs to: 0 isolated, >= 2 an articulation point
//   edge_component[v] = the smallest vertex of v's 2-edge-connected component
// Row shards are not supported: the kernel reads the forest's words of every column of a row.
#ifndef GRAPHLILY_HIP_APP_BICC_H_
#define GRAPHLILY_HIP_APP_BICC_H_

#include "graphlily/app/pattern_app.h"

#include <vector>

namespace graphlily {
namespace app {

class BiconnectedComponents : public app::PatternApp {
private:
    CSRMatrix<float> graph_;
    std::vector<uint32_t> blocks_, vertex_blocks_, edge_components_;
    uint64_t num_blocks_ = 0, num_articulation_ = 0, num_bridges_ = 0, depth_ = 0, launches_ = 0, num_trees_ = 0;

    // get_nnz() counts the entries of the symmetric matrix: twice the undirected edges
    CSRMatrix<float> prepare(CSRMatrix<float> &padded) override {
        graph_ = graphlily::io::util_symmetrize_simple(padded, degrees_);
        return graph_;
    }

public:
    typedef std::vector<uint32_t, aligned_allocator<uint32_t>> aligned_block_vec_t;

    BiconnectedComponents(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : PatternApp("BiconnectedComponents", num_channels, spmv_out_buf_len, vec_buf_len) {}

    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric simple matrix blocks() is aligned with

    // the block label of every entry's edge; leaves blocks(), vertex_blocks(), num_blocks(), num_articulation_points(),
    // num_bridges(), num_trees(), depth(), launches() and, with edge_components, edge_components().  Padding vertices are
    // isolated: they belong to no block and are trees of their own, which num_trees() does not count.  The call waits for the device.
    aligned_block_vec_t run(bool edge_components = false) {
        require_sent("run()");
        const size_t n = matrix_num_rows_, nnz = graph_.adj_indices.size();
        DeviceBuffer block(sizeof(uint32_t) * (nnz ? nnz : 1)), vb(sizeof(uint32_t) * (n ? n : 1));
        DeviceBuffer ec = edge_components ? DeviceBuffer(sizeof(uint32_t) * (n ? n : 1)) : DeviceBuffer();
        uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
        SpMV_->bicc(block, vb, ec, stats);
        aligned_block_vec_t out(nnz);
        if (nnz) block.download(out.data(), sizeof(uint32_t) * nnz);
        blocks_.assign(out.begin(), out.end());
        vertex_blocks_.assign(n, 0);
        if (n) vb.download(vertex_blocks_.data(), sizeof(uint32_t) * n);
        edge_components_.assign(edge_components ? n : 0, 0);
        if (edge_components && n) ec.download(edge_components_.data(), sizeof(uint32_t) * n);
        num_blocks_ = stats[0];
        num_articulation_ = stats[1];
        num_bridges_ = stats[2];
        depth_ = stats[3];
        launches_ = stats[4];
        num_trees_ = stats[5] - (n - n_real_);
        return out;
    }
    const std::vector<uint32_t> &blocks() const { return blocks_; }
    const std::vector<uint32_t> &vertex_blocks() const { return vertex_blocks_; }
    const std::vector<uint32_t> &edge_components() const { return edge_components_; }    // empty unless run(true)
    uint64_t num_blocks() const { return num_blocks_; }
    uint64_t num_articulation_points() const { return num_articulation_; }
    uint64_t num_bridges() const { return num_bridges_; }
    uint64_t num_trees() const { return num_trees_; }                // over the real vertices
    uint64_t depth() const { return depth_; }                        // the largest level of the BFS forest
    uint64_t launches() const { return launches_; }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_BICC_H_
