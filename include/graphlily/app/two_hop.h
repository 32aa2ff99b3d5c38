// graphlily/app/two_hop.h -- two-hop neighbourhoods of a simple undirected graph over the MI355X backend (an extension: the
// reference has no such driver; the C++ twin of app.TwoHop), with the conventions of the drivers next to it: print and exit on
// error, device-resident buffers.  One SpGEMMModule (graphlily/module/spgemm_module.h) holds ONE plan of the graph
// and two masks.  The matrix is read as KCore reads it (graphlily::io::util_symmetrize_simple): duplicates, the diagonal,
// zero-valued entries and direction are ignored.
//   run_paths()       the number of paths of length two between every pair of DISTINCT vertices that has one, adjacent or not:
//                     A A under (+,x) on all-ones values, masked by the complement of the identity
//   run_candidates()  the pattern of the pairs at distance exactly two: A A under (||,&&), masked by the complement of A + I
#ifndef GRAPHLILY_HIP_APP_TWO_HOP_H_
#define GRAPHLILY_HIP_APP_TWO_HOP_H_

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spgemm_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <algorithm>
#include <string>
#include <vector>

namespace graphlily {
namespace app {

class TwoHop : public app::ModuleCollection {
private:
    graphlily::module::SpGEMMModule *SpGEMM_;
    CSRMatrix<float> graph_;
    std::vector<uint32_t> degrees_;
    bool sent_ = false;

    // the identity, with_graph: joined with the graph (whose rows ascend and hold no diagonal entry)
    CSRMatrix<float> mask_(bool with_graph) const {
        const uint32_t n = graph_.num_rows;
        CSRMatrix<float> m{n, n, {}, {}, std::vector<uint32_t>((size_t)n + 1, 0)};
        for (uint32_t v = 0; v < n; v++) {
            if (with_graph) m.adj_indices.insert(m.adj_indices.end(), graph_.adj_indices.begin() + graph_.adj_indptr[v], graph_.adj_indices.begin() + graph_.adj_indptr[v + 1]);
            m.adj_indices.push_back(v);
            std::inplace_merge(m.adj_indices.begin() + m.adj_indptr[v], m.adj_indices.end() - 1, m.adj_indices.end());
            m.adj_indptr[v + 1] = (uint32_t)m.adj_indices.size();
        }
        m.adj_data.assign(m.adj_indices.size(), 1.0f);
        return m;
    }
    CSRMatrix<float> run_(graphlily::SemiringType semiring, size_t slot) {
        if (!sent_) {
            printf("TwoHop::run: send_matrix_host_to_device first\n");
            exit(EXIT_FAILURE);
        }
        SpGEMM_->set_semiring(semiring);
        SpGEMM_->set_mask_type(graphlily::kMaskWriteToZero, slot);
        SpGEMM_->run();
        return SpGEMM_->send_results_device_to_host();
    }

public:
    TwoHop() {
        SpGEMM_ = new graphlily::module::SpGEMMModule();
        add_module(SpGEMM_);
    }

    uint32_t num_vertices() const { return graph_.num_rows; }
    const CSRMatrix<float> &graph() const { return graph_; }        // the symmetric matrix the results are over
    const std::vector<uint32_t> &degrees() const { return degrees_; }
    const uint64_t *stats() const { return SpGEMM_->stats(); }      // of the last run's symbolic call

    void load_and_format_matrix(std::string csr_float_npz_path) {
        CSRMatrix<float> raw = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        graph_ = graphlily::io::util_symmetrize_simple(raw, degrees_);
        SpGEMM_->load_and_format_matrices(graph_);
        SpGEMM_->load_mask_matrix(mask_(false), 0);
        SpGEMM_->load_mask_matrix(mask_(true), 1);
        sent_ = false;
    }
    void send_matrix_host_to_device() {
        SpGEMM_->send_matrices_host_to_device();
        sent_ = true;
    }
    CSRMatrix<float> run_paths() { return run_(graphlily::ArithmeticSemiring, 0); }
    CSRMatrix<float> run_candidates() { return run_(graphlily::LogicalSemiring, 1); }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_TWO_HOP_H_
