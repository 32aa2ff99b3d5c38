// graphlily::app::TopologicalOrder driven from C++: level, dist, parent and the canonical order are written as raw 32-bit words for
// tests/test_gpu_topo.py to compare with the Python driver's, the counts are printed, and what ties the outputs together is checked
// here against Kahn's algorithm run on the host over the successors' rows, with the predecessors visited in ascending order.
//   topo_driver graph.npz out_dir [weighted: 0 (default), 1] [reverse: 0 (default), 1]
//   g++ -std=c++11 -I<repo>/include tests/cpp/topo_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/topo.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

template <typename T>
static bool write_words(const std::string &path, const std::vector<T> &words) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(words.data(), sizeof(T), words.size(), f) != words.size()) { printf("cannot write %s\n", path.c_str()); return false; }
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir [weighted] [reverse]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const bool weighted = argc > 3 && atoi(argv[3]) != 0, reverse = argc > 4 && atoi(argv[4]) != 0;
    graphlily::app::TopologicalOrder topo(graphlily::num_hbm_channels, 1024, 256);
    topo.set_target("hw");
    topo.set_up_runtime("unused.xclbin");
    topo.load_and_format_matrix(npz, true, weighted);
    topo.send_matrix_host_to_device();
    auto level = topo.run(reverse, true);
    const size_t n = topo.num_vertices(), nr = topo.num_real_vertices();
    if (level.size() != n || topo.level().size() != n || (weighted && (topo.dist().size() != n || topo.parent().size() != n))) {
        printf("size mismatch\n");
        return 1;
    }
    // Kahn's algorithm on the host; reverse: the two matrices change places
    const CSRMatrix<float> &in = reverse ? topo.graph_out() : topo.graph(), &succ = reverse ? topo.graph() : topo.graph_out();
    std::vector<uint32_t> pending(n, 0), want(n, 0xffffffffu), wparent(n, 0xffffffffu), queue;
    std::vector<float> wdist(n);
    const uint32_t nan_bits = 0x7fc00000u;
    for (size_t v = 0; v < n; v++) {
        memcpy(&wdist[v], &nan_bits, 4);
        pending[v] = in.adj_indptr[v + 1] - in.adj_indptr[v];
        if (!pending[v]) queue.push_back((uint32_t)v);
    }
    for (size_t head = 0, lvl = 0; head < queue.size(); lvl++) {
        for (const size_t stop = queue.size(); head < stop; head++) {
            const uint32_t v = queue[head];
            want[v] = (uint32_t)lvl;
            wdist[v] = 0.0f;
            for (uint32_t j = in.adj_indptr[v]; j < in.adj_indptr[v + 1]; j++) {      // ascending u: the first to attain the maximum stays
                const uint32_t u = in.adj_indices[j];
                const float cand = wdist[u] + in.adj_data[j];
                if (j == in.adj_indptr[v] || cand > wdist[v]) {
                    wdist[v] = cand;
                    wparent[v] = u;
                }
            }
            for (uint32_t j = succ.adj_indptr[v]; j < succ.adj_indptr[v + 1]; j++)
                if (--pending[succ.adj_indices[j]] == 0) queue.push_back(succ.adj_indices[j]);
        }
    }
    int bad = 0;
    for (size_t v = 0; v < n; v++) {
        if (want[v] != level[v] && bad++ < 5) printf("vertex %zu has level %u, Kahn's algorithm on the host gives %u\n", v, level[v], want[v]);
        if (!weighted) continue;
        if (memcmp(&wdist[v], &topo.dist()[v], 4) != 0 && bad++ < 5) printf("vertex %zu has dist %g, the host gives %g\n", v, topo.dist()[v], wdist[v]);
        if (wparent[v] != topo.parent()[v] && bad++ < 5) printf("vertex %zu has parent %u, the host gives %u\n", v, topo.parent()[v], wparent[v]);
    }
    uint64_t members = 0;
    for (uint64_t c : topo.level_sizes()) members += c;
    if (members != topo.num_peeled() || topo.order().size() != topo.num_peeled() || topo.position().size() != nr) {
        printf("%llu members of %llu levels, %llu peeled, %zu ordered\n", (unsigned long long)members, (unsigned long long)topo.num_levels(),
               (unsigned long long)topo.num_peeled(), topo.order().size());
        bad++;
    }
    for (size_t i = 1; i < topo.order().size(); i++) {
        const uint32_t a = topo.order()[i - 1], b = topo.order()[i];
        if ((level[a] > level[b] || (level[a] == level[b] && a >= b)) && bad++ < 5) printf("order[%zu] = %u does not go before order[%zu] = %u\n", i - 1, a, i, b);
    }
    std::vector<uint32_t> path = topo.critical_path();
    if (weighted && topo.num_peeled()) {                        // a path of stored edges whose f32 running sum is critical_length()
        float sum = 0.0f;
        for (size_t i = path.size(); i-- > 1;) {
            const uint32_t v = path[i - 1], u = path[i];
            uint32_t j = in.adj_indptr[v];
            while (j < in.adj_indptr[v + 1] && in.adj_indices[j] != u) j++;
            if (j == in.adj_indptr[v + 1]) { printf("the critical path uses %u -> %u, which is no stored edge\n", u, v); bad++; break; }
            sum += in.adj_data[j];
        }
        const float length = topo.critical_length();
        if (path.empty() || memcmp(&sum, &length, 4) != 0) { printf("the critical path sums to %g, critical_length() is %g\n", sum, length); bad++; }
    }
    std::vector<uint32_t> words(level.begin(), level.end());
    if (!write_words(out + "/cpp_level.bin", words) || !write_words(out + "/cpp_order.bin", topo.order())) return 2;
    if (weighted && (!write_words(out + "/cpp_dist.bin", topo.dist()) || !write_words(out + "/cpp_parent.bin", topo.parent()) ||
                     !write_words(out + "/cpp_path.bin", path))) return 2;
    printf("symmetric: %d\npeeled: %llu\nis_dag: %d\nlevels: %llu\nwidest: %llu\n", topo.symmetric() ? 1 : 0, (unsigned long long)topo.num_peeled(),
           topo.is_dag() ? 1 : 0, (unsigned long long)topo.num_levels(), (unsigned long long)topo.widest());
    if (weighted) printf("critical_length: %.9g\n", (double)topo.critical_length());
    if (!bad) printf("TopologicalOrder::run OK\n");
    return bad ? 1 : 0;
}
