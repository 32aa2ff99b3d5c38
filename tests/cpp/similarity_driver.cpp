// graphlily::app::Similarity driven from C++: the pairs, the common-neighbour counts, the two fixed-point sums and every measure
// are written as raw words for tests/test_gpu_sim.py to compare with the Python driver's, the counts are printed, and the integers
// are checked here against a merge of the two sorted rows on the host.
//   similarity_driver graph.npz out_dir [number of pairs: 0 (default) = every edge {u, v}, u < v; k: the pairs ((7 i) mod n_real, (11 i + 3) mod n_real)]
//   g++ -std=c++11 -I<repo>/include tests/cpp/similarity_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/similarity.h"

#include <cstdio>
#include <cstdlib>
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
    if (argc < 3) { printf("usage: %s graph.npz out_dir [pairs]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const size_t count = argc > 3 ? (size_t)atoi(argv[3]) : 0;
    typedef graphlily::app::Similarity Sim;
    Sim sim(graphlily::num_hbm_channels, 1024, 256);
    sim.set_target("hw");
    sim.set_up_runtime("unused.xclbin");
    sim.load_and_format_matrix(npz, true);
    sim.send_matrix_host_to_device();
    const size_t nr = sim.num_real_vertices();
    if (count) {
        Sim::pairs_t pairs;
        for (size_t i = 0; i < count; i++) pairs.push_back(std::make_pair((uint32_t)((7 * i) % nr), (uint32_t)((11 * i + 3) % nr)));
        sim.run(pairs, true, true);
    } else {
        sim.run_edges(true, true);
    }
    const Sim::pairs_t &pairs = sim.pairs();
    const size_t m = pairs.size();
    if (sim.common().size() != m || sim.adamic_adar_sums().size() != m || sim.resource_allocation_sums().size() != m) {
        printf("size mismatch\n");
        return 1;
    }
    const CSRMatrix<float> &g = sim.graph();
    int bad = 0;
    std::vector<uint32_t> flat(2 * m);
    for (size_t i = 0; i < m; i++) {
        const uint32_t u = pairs[i].first, v = pairs[i].second;
        flat[2 * i] = u;
        flat[2 * i + 1] = v;
        uint32_t a = g.adj_indptr[u], b = g.adj_indptr[v], c = 0;
        uint64_t aa = 0, ra = 0;
        while (a < g.adj_indptr[u + 1] && b < g.adj_indptr[v + 1]) {
            const uint32_t x = g.adj_indices[a], y = g.adj_indices[b];
            if (x == y) {
                c++;
                aa += sim.adamic_adar_weights()[x];
                ra += sim.resource_allocation_weights()[x];
            }
            a += x <= y;
            b += y <= x;
        }
        if ((sim.common()[i] != c || sim.adamic_adar_sums()[i] != aa || sim.resource_allocation_sums()[i] != ra) && bad++ < 5)
            printf("pair %zu = (%u, %u): {%u, %llu, %llu}, the host merge gives {%u, %llu, %llu}\n", i, u, v, sim.common()[i],
                   (unsigned long long)sim.adamic_adar_sums()[i], (unsigned long long)sim.resource_allocation_sums()[i], c,
                   (unsigned long long)aa, (unsigned long long)ra);
    }
    const char *names[8] = {"common", "jaccard", "overlap", "sorensen", "cosine", "preferential_attachment", "adamic_adar", "resource_allocation"};
    for (int k = 0; k < 8; k++)
        if (!write_words(out + "/cpp_score_" + names[k] + ".bin", sim.score((Sim::Measure)k))) return 2;
    if (!write_words(out + "/cpp_pairs.bin", flat) || !write_words(out + "/cpp_common.bin", sim.common()) ||
        !write_words(out + "/cpp_aa.bin", sim.adamic_adar_sums()) || !write_words(out + "/cpp_ra.bin", sim.resource_allocation_sums()) ||
        !write_words(out + "/cpp_aa_table.bin", sim.adamic_adar_weights()) || !write_words(out + "/cpp_ra_table.bin", sim.resource_allocation_weights()))
        return 2;
    printf("pairs: %zu\nshift: %d\nlaunches: %llu\ndeferred: %llu\n", m, sim.shift(), (unsigned long long)sim.launches(), (unsigned long long)sim.deferred());
    if (!bad) printf("Similarity::run OK\n");
    return bad ? 1 : 0;
}
