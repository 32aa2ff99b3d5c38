// graphlily::app::ShortestPaths driven from C++: dist and parent are written as raw 32-bit words for tests/test_gpu_sssp_delta.py
// to compare with the Python driver's, the counts are printed, and the distances are checked here against Dijkstra's algorithm
// run in f32 on the host over the successors' rows, the parents against their definition over the predecessors' rows.
//   shortest_paths_driver graph.npz out_dir [weighted: 1 (default), 0] [delta: 0 (default: the driver's), > 0] [source ...: 0]
//   g++ -std=c++11 -I<repo>/include tests/cpp/shortest_paths_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/shortest_paths.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <queue>
#include <string>
#include <utility>
#include <vector>

template <typename T>
static bool write_words(const std::string &path, const std::vector<T> &words) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(words.data(), sizeof(T), words.size(), f) != words.size()) { printf("cannot write %s\n", path.c_str()); return false; }
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir [weighted] [delta] [source ...]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const bool weighted = argc <= 3 || atoi(argv[3]) != 0;
    const float delta = argc > 4 ? (float)atof(argv[4]) : 0.0f;
    std::vector<uint32_t> sources;
    for (int i = 5; i < argc; i++) sources.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
    if (sources.empty()) sources.push_back(0);
    graphlily::app::ShortestPaths sp(graphlily::num_hbm_channels, 1024, 256);
    sp.set_target("hw");
    sp.set_up_runtime("unused.xclbin");
    sp.load_and_format_matrix(npz, true, weighted);
    sp.send_matrix_host_to_device();
    auto dist = sp.run(sources, delta, true);
    const size_t n = sp.num_vertices();
    if (dist.size() != n || sp.dist().size() != n || sp.parent().size() != n) { printf("size mismatch\n"); return 1; }
    // Dijkstra's algorithm in f32 on the host
    const CSRMatrix<float> &in = sp.graph(), &succ = sp.graph_out();
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> want(n, inf);
    typedef std::pair<float, uint32_t> item_t;
    std::priority_queue<item_t, std::vector<item_t>, std::greater<item_t>> heap;
    for (uint32_t s : sources) {
        want[s] = 0.0f;
        heap.push(std::make_pair(0.0f, s));
    }
    while (!heap.empty()) {
        const item_t top = heap.top();
        heap.pop();
        if (top.first > want[top.second]) continue;
        for (uint32_t j = succ.adj_indptr[top.second]; j < succ.adj_indptr[top.second + 1]; j++) {
            const float cand = top.first + succ.adj_data[j];
            if (cand < want[succ.adj_indices[j]]) {
                want[succ.adj_indices[j]] = cand;
                heap.push(std::make_pair(cand, succ.adj_indices[j]));
            }
        }
    }
    int bad = 0;
    uint64_t reached = 0, orphans = 0;
    std::vector<bool> is_source(n, false);
    for (uint32_t s : sources) is_source[s] = true;
    for (size_t v = 0; v < n; v++) {
        if (memcmp(&want[v], &dist[v], 4) != 0 && bad++ < 5) printf("vertex %zu has dist %g, Dijkstra on the host gives %g\n", v, dist[v], want[v]);
        uint32_t wparent = 0xffffffffu;                            // ascending u: the first that fits is the smallest
        if (want[v] < inf) reached++;
        if (is_source[v]) wparent = (uint32_t)v;
        for (uint32_t j = in.adj_indptr[v]; j < in.adj_indptr[v + 1] && want[v] < inf && wparent == 0xffffffffu; j++) {
            const uint32_t u = in.adj_indices[j];
            const float through = want[u] + in.adj_data[j];
            if (want[u] < want[v] && through == want[v]) wparent = u;
        }
        if (want[v] < inf && wparent == 0xffffffffu) orphans++;
        if (wparent != sp.parent()[v] && bad++ < 5) printf("vertex %zu has parent %u, the host gives %u\n", v, sp.parent()[v], wparent);
    }
    if (reached != sp.reached() || orphans != sp.orphans()) {
        printf("%llu reached and %llu orphans, the host counts %llu and %llu\n", (unsigned long long)sp.reached(), (unsigned long long)sp.orphans(),
               (unsigned long long)reached, (unsigned long long)orphans);
        bad++;
    }
    if (!write_words(out + "/cpp_dist.bin", sp.dist()) || !write_words(out + "/cpp_parent.bin", sp.parent())) return 2;
    printf("symmetric: %d\nreached: %llu\norphans: %llu\n", sp.symmetric() ? 1 : 0, (unsigned long long)sp.reached(), (unsigned long long)sp.orphans());
    if (!bad) printf("ShortestPaths::run OK\n");
    return bad ? 1 : 0;
}
