// graphlily::app::QuotientGraph driven from C++: the graph is contracted by the labelling label[v] = 5 (v / 5), read undirected
// and directed, and every result array is written as raw 32-bit words for tests/test_gpu_contract.py to compare with the Python
// driver's.  What ties the outputs together is checked here: the offsets ascend from 0 to nnz, the columns of every row ascend and
// avoid the diagonal, part follows the labels, and the weights outside plus the weight inside are the graph's entries.
//   quotient_driver graph.npz out_dir
//   g++ -std=c++11 -I<repo>/include tests/cpp/quotient_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/quotient.h"

#include <cstdio>
#include <cstdlib>
#include <string>

static bool dump(const std::string &path, const std::vector<uint32_t> &words) {
    FILE *f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(words.data(), sizeof(uint32_t), words.size(), f) == words.size();
    if (f) fclose(f);
    if (!ok) printf("cannot write %s\n", path.c_str());
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    int bad = 0;
    for (int directed = 0; directed < 2; directed++) {
        graphlily::app::QuotientGraph q(graphlily::num_hbm_channels, 1024, 256);
        q.set_target("hw");
        q.set_up_runtime("unused.xclbin");
        q.load_and_format_matrix(npz, true, directed);
        q.send_matrix_host_to_device();
        std::vector<uint32_t> labels(q.num_real_vertices());
        for (size_t v = 0; v < labels.size(); v++) labels[v] = (uint32_t)(v / 5 * 5);
        const CSRMatrix<float> &c = q.run(labels);
        const size_t k = q.num_groups();
        if (c.adj_indptr.size() != k + 1 || c.adj_indptr[0] != 0 || c.adj_indptr[k] != c.adj_indices.size() || q.tot().size() != k) { printf("sizes are off\n"); return 1; }
        unsigned long long outside = 0;
        for (size_t a = 0; a < k; a++)
            for (uint32_t j = c.adj_indptr[a]; j < c.adj_indptr[a + 1]; j++) {
                if ((c.adj_indices[j] == a || c.adj_indices[j] >= k || (j > c.adj_indptr[a] && c.adj_indices[j - 1] >= c.adj_indices[j])) && bad++ < 5)
                    printf("row %zu: column %u does not belong or does not ascend\n", a, c.adj_indices[j]);
                outside += q.weights()[j];
            }
        for (size_t v = 0; v < labels.size(); v++)
            if (q.community_of()[v] != v / 5 && bad++ < 5) printf("part[%zu] = %u\n", v, q.community_of()[v]);
        if (outside + q.inside_weight() != q.graph().adj_indices.size() || q.directed() != (directed != 0)) { printf("the weights do not add up\n"); bad++; }
        const std::string stem = out + (directed ? "/cpp_directed_" : "/cpp_undirected_");
        if (!dump(stem + "indptr.bin", c.adj_indptr) || !dump(stem + "indices.bin", c.adj_indices) || !dump(stem + "weights.bin", q.weights()) ||
            !dump(stem + "tot.bin", q.tot()) || !dump(stem + "part.bin", q.community_of()))
            return 2;
        printf("%s: %zu groups, nnz %zu, inside %llu, paths %u %u %u\n", directed ? "directed" : "undirected", k, c.adj_indices.size(),
               (unsigned long long)q.inside_weight(), q.paths()[0], q.paths()[1], q.paths()[2]);
    }
    if (!bad) printf("QuotientGraph OK\n");
    return bad ? 1 : 0;
}
