// graphlily::app::ClosenessCentrality driven from C++: far, reach, harmonic, closeness and hops are written as raw words for
// tests/test_gpu_msbfs.py to compare with the Python driver's, the counts are printed, and the arrays are checked here against one
// breadth-first search per source on the host, with the harmonic sum in the device's order (per batch of 64, levels ascending).
//   closeness_driver graph.npz out_dir [number of sources: 0 (default) = every real vertex; k: the vertices (7 i) mod n_real] [reverse: 0 (default), 1]
//   g++ -std=c++11 -I<repo>/include tests/cpp/closeness_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/closeness.h"

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
    if (argc < 3) { printf("usage: %s graph.npz out_dir [sources] [reverse]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const size_t count = argc > 3 ? (size_t)atoi(argv[3]) : 0;
    const bool reverse = argc > 4 && atoi(argv[4]) != 0;
    graphlily::app::ClosenessCentrality cc(graphlily::num_hbm_channels, 1024, 256);
    cc.set_target("hw");
    cc.set_up_runtime("unused.xclbin");
    cc.load_and_format_matrix(npz, true);
    cc.send_matrix_host_to_device();
    const size_t n = cc.num_vertices(), nr = cc.num_real_vertices();
    std::vector<uint32_t> sources;
    for (size_t i = 0; i < count; i++) sources.push_back((uint32_t)((7 * i) % nr));      // (distinct while count <= n_real and 7 does not divide it)
    std::vector<double> closeness = cc.run(sources, reverse, true, true);
    const std::vector<uint32_t> &src = cc.sources();
    const size_t k = src.size();
    if (closeness.size() != n || cc.far().size() != n || cc.reach().size() != n || cc.harmonic().size() != n || cc.hops().size() != k * n) {
        printf("size mismatch\n");
        return 1;
    }
    // one search per source over the successors' rows (reverse: the predecessors')
    const CSRMatrix<float> &walk = reverse ? cc.graph() : cc.graph_out();
    std::vector<uint32_t> hops(k * n, 0xffffffffu), queue;
    int bad = 0;
    uint64_t diameter = 0;
    for (size_t j = 0; j < k; j++) {
        uint32_t *h = hops.data() + j * n;
        queue.assign(1, src[j]);
        h[src[j]] = 0;
        uint64_t reached = 0, total = 0, ecc = 0;
        for (size_t head = 0; head < queue.size(); head++) {
            const uint32_t u = queue[head];
            for (uint32_t e = walk.adj_indptr[u]; e < walk.adj_indptr[u + 1]; e++) {
                const uint32_t v = walk.adj_indices[e];
                if (h[v] != 0xffffffffu) continue;
                h[v] = h[u] + 1;
                reached++;
                total += h[v];
                ecc = h[v];
                queue.push_back(v);
            }
        }
        diameter = std::max(diameter, ecc);
        if ((cc.source_reach()[j] != reached || cc.source_far()[j] != total || cc.eccentricity()[j] != ecc) && bad++ < 5)
            printf("source %u: {%llu, %llu, %llu}, the host search gives {%llu, %llu, %llu}\n", src[j], (unsigned long long)cc.source_reach()[j],
                   (unsigned long long)cc.source_far()[j], (unsigned long long)cc.eccentricity()[j], (unsigned long long)reached,
                   (unsigned long long)total, (unsigned long long)ecc);
    }
    for (size_t i = 0; i < k * n; i++)
        if (hops[i] != cc.hops()[i] && bad++ < 5) printf("hops[%zu, %zu] is %u, the host search gives %u\n", i / n, i % n, cc.hops()[i], hops[i]);
    std::vector<uint64_t> far(n, 0);
    std::vector<uint32_t> reach(n, 0), c(n);
    std::vector<double> harmonic(n, 0.0);
    for (size_t b = 0; b < k; b += 64) {
        const size_t stop = std::min(k, b + 64);
        for (uint64_t d = 1; d <= diameter; d++) {
            std::fill(c.begin(), c.end(), 0u);
            for (size_t j = b; j < stop; j++)
                for (size_t v = 0; v < n; v++) c[v] += hops[j * n + v] == d;
            for (size_t v = 0; v < n; v++) {
                if (!c[v]) continue;
                far[v] += (uint64_t)c[v] * d;
                reach[v] += c[v];
                harmonic[v] = harmonic[v] + (double)c[v] / (double)d;
            }
        }
    }
    for (size_t v = 0; v < n; v++) {
        if (far[v] != cc.far()[v] && bad++ < 5) printf("vertex %zu has far %llu, the host gives %llu\n", v, (unsigned long long)cc.far()[v], (unsigned long long)far[v]);
        if (reach[v] != cc.reach()[v] && bad++ < 5) printf("vertex %zu has reach %u, the host gives %u\n", v, cc.reach()[v], reach[v]);
        if (memcmp(&harmonic[v], &cc.harmonic()[v], 8) != 0 && bad++ < 5) printf("vertex %zu has harmonic %.17g, the host gives %.17g\n", v, cc.harmonic()[v], harmonic[v]);
    }
    if (cc.diameter() != diameter) { printf("diameter %llu, the host gives %llu\n", (unsigned long long)cc.diameter(), (unsigned long long)diameter); bad++; }
    if (!write_words(out + "/cpp_far.bin", cc.far()) || !write_words(out + "/cpp_reach.bin", cc.reach()) ||
        !write_words(out + "/cpp_harmonic.bin", cc.harmonic()) || !write_words(out + "/cpp_closeness.bin", closeness) ||
        !write_words(out + "/cpp_hops.bin", cc.hops()) || !write_words(out + "/cpp_eccentricity.bin", cc.eccentricity()))
        return 2;
    printf("symmetric: %d\nsources: %zu\nbatches: %llu\nlevels: %llu\ndiameter: %llu\nradius: %llu\ncenter: %zu\nperiphery: %zu\n", cc.symmetric() ? 1 : 0, k,
           (unsigned long long)cc.batches(), (unsigned long long)cc.levels(), (unsigned long long)cc.diameter(), (unsigned long long)cc.radius(),
           cc.center().size(), cc.periphery().size());
    if (!bad) printf("ClosenessCentrality::run OK\n");
    return bad ? 1 : 0;
}
