// graphlily::app::StronglyConnectedComponents driven from C++: the labels are written as raw 32-bit words for
// tests/test_gpu_scc.py to compare with the Python driver's, the counts and a checksum are printed, and what ties the outputs
// together is checked here: label[label[v]] == label[v] <= v, the component sizes add up to the real vertices, and the classes are
// those of Tarjan's algorithm run on the host over the successors' rows (iterative, so that a long path does not overflow the stack).
//   scc_driver graph.npz out_dir [order: largest_first (default), natural, random] [seed: 0]
//   g++ -std=c++11 -I<repo>/include tests/cpp/scc_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/scc.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

// -> for every vertex the smallest vertex of its strongly connected component; row v of `out` holds the successors of v
static std::vector<uint32_t> tarjan_min_labels(const CSRMatrix<float> &out, size_t n) {
    const uint32_t none = 0xffffffffu;
    std::vector<uint32_t> index(n, none), low(n, 0), label(n, none), stack;
    std::vector<bool> on_stack(n, false);
    std::vector<std::pair<uint32_t, uint32_t>> calls;      // (vertex, next entry of its row)
    uint32_t counter = 0;
    for (size_t s = 0; s < n; s++) {
        if (index[s] != none) continue;
        calls.push_back(std::make_pair((uint32_t)s, s < out.num_rows ? out.adj_indptr[s] : 0u));
        while (!calls.empty()) {
            const uint32_t v = calls.back().first;
            if (index[v] == none) {
                index[v] = low[v] = counter++;
                stack.push_back(v);
                on_stack[v] = true;
            }
            const uint32_t end = v < out.num_rows ? out.adj_indptr[v + 1] : 0u;
            bool descended = false;
            while (calls.back().second < end) {
                const uint32_t w = out.adj_indices[calls.back().second++];
                if (index[w] == none) {
                    calls.push_back(std::make_pair(w, w < out.num_rows ? out.adj_indptr[w] : 0u));
                    descended = true;
                    break;
                }
                if (on_stack[w]) low[v] = std::min(low[v], index[w]);
            }
            if (descended) continue;
            calls.pop_back();
            if (!calls.empty()) low[calls.back().first] = std::min(low[calls.back().first], low[v]);
            if (low[v] != index[v]) continue;
            size_t from = stack.size();
            uint32_t smallest = v;
            do {
                from--;
                smallest = std::min(smallest, stack[from]);
            } while (stack[from] != v);
            for (size_t i = from; i < stack.size(); i++) {
                label[stack[i]] = smallest;
                on_stack[stack[i]] = false;
            }
            stack.resize(from);
        }
    }
    return label;
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir [order] [seed]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2], order = argc > 3 ? argv[3] : "largest_first";
    const uint32_t seed = argc > 4 ? (uint32_t)strtoul(argv[4], nullptr, 10) : 0u;
    graphlily::app::StronglyConnectedComponents scc(graphlily::num_hbm_channels, 1024, 256);
    scc.set_target("hw");
    scc.set_up_runtime("unused.xclbin");
    scc.load_and_format_matrix(npz, true);
    scc.send_matrix_host_to_device();
    auto label = scc.run(order, seed);
    int bad = 0;
    const size_t n = scc.num_vertices();
    if (label.size() != n || scc.labels().size() != n || scc.degrees().size() != n || (order != "natural" && scc.priorities().size() != n)) {
        printf("size mismatch\n");
        return 1;
    }
    unsigned long long checksum = 0, members = 0;
    for (size_t v = 0; v < n; v++) {
        checksum = checksum * 1000003ull + label[v] + 1ull;          // (mod 2^64: tests/test_gpu_scc.py computes the same)
        if ((label[v] > v || label[label[v] < n ? label[v] : v] != label[v]) && bad++ < 5)
            printf("vertex %zu has label %u, which is above it or is not its own label\n", v, label[v]);
    }
    const std::vector<uint32_t> want = tarjan_min_labels(scc.graph_out(), n);
    for (size_t v = 0; v < n; v++)
        if (want[v] != label[v] && bad++ < 5) printf("vertex %zu has label %u, Tarjan's algorithm on the host gives %u\n", v, label[v], want[v]);
    for (uint64_t c : scc.component_sizes()) members += c;
    if (members != scc.num_real_vertices() || scc.component_labels().size() != scc.num_components() ||
        scc.component_sizes().size() != scc.num_components()) {
        printf("%llu members of %llu components, %u real vertices\n", members, (unsigned long long)scc.num_components(), scc.num_real_vertices());
        bad++;
    }
    const std::string p = out + "/cpp_label.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(label.data(), sizeof(label[0]), label.size(), f) != label.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("symmetric: %d\ncomponents: %llu\nlargest: %llu\nis_dag: %d\npasses: %llu\ntrimmed: %llu\nchecksum: %llu\n", scc.symmetric() ? 1 : 0,
           (unsigned long long)scc.num_components(), (unsigned long long)scc.largest_component(), scc.is_dag() ? 1 : 0,
           (unsigned long long)scc.passes(), (unsigned long long)scc.trimmed(), checksum);
    if (!bad) printf("StronglyConnectedComponents::run OK\n");
    return bad ? 1 : 0;
}
