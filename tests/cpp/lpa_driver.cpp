// graphlily::app::LabelPropagation driven from C++: the labels and the colours are written as raw 32-bit words for
// tests/test_gpu_lpa.py to compare with the Python driver's, the stats, the communities, the modularity and a checksum are printed,
// and what ties the outputs together is checked here: every label is an initial label, an isolated vertex keeps its own, the
// colouring is proper, the community sizes add up to the real vertices, and -- if the run converged -- every vertex with a
// neighbour carries a label that a maximum number of its neighbours carry.
//   lpa_driver graph.npz out_dir [order: largest_first (default), natural, random, smallest_last] [seed: -1 (default: none) or >= 0]
//              [max_sweeps: 100] [synchronous: 0 (default) or 1]
//   g++ -std=c++11 -I<repo>/include tests/cpp/lpa_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/lpa.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir [order] [seed] [max_sweeps] [synchronous]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2], order = argc > 3 ? argv[3] : "largest_first";
    const long seed = argc > 4 ? atol(argv[4]) : -1, max_sweeps = argc > 5 ? atol(argv[5]) : 100;
    const bool synchronous = argc > 6 && atoi(argv[6]) != 0;
    graphlily::app::LabelPropagation lpa(graphlily::num_hbm_channels, 1024, 256);
    lpa.set_target("hw");
    lpa.set_up_runtime("unused.xclbin");
    lpa.load_and_format_matrix(npz, true);
    lpa.send_matrix_host_to_device();
    auto label = lpa.run((uint32_t)max_sweeps, order, seed >= 0, seed >= 0 ? (uint32_t)seed : 0u, synchronous);
    int bad = 0;
    const size_t n = lpa.num_vertices();
    if (label.size() != n || lpa.labels().size() != n || lpa.colors().size() != (synchronous ? 0 : n)) {
        printf("size mismatch\n");
        return 1;
    }
    const CSRMatrix<float> &g = lpa.graph();
    std::vector<uint32_t> start(lpa.initial());
    if (start.empty()) for (size_t v = 0; v < n; v++) start.push_back((uint32_t)v);
    const std::set<uint32_t> known(start.begin(), start.end());
    unsigned long long checksum = 0, members = 0;
    for (size_t v = 0; v < n; v++) {
        checksum = checksum * 1000003ull + label[v] + 1ull;          // (mod 2^64: tests/test_gpu_lpa.py computes the same)
        if (!known.count(label[v]) && bad++ < 5) printf("vertex %zu carries %u, which no vertex started with\n", v, label[v]);
        const uint32_t b = g.adj_indptr[v], e = g.adj_indptr[v + 1];
        if (b == e) {
            if (label[v] != start[v] && bad++ < 5) printf("vertex %zu has no neighbour and carries %u, not %u\n", v, label[v], start[v]);
            continue;
        }
        std::map<uint32_t, uint32_t> cnt;
        for (uint32_t j = b; j < e; j++) {
            const uint32_t u = g.adj_indices[j];
            cnt[label[u]]++;
            if (!synchronous && lpa.colors()[u] == lpa.colors()[v] && bad++ < 5) printf("edge (%zu, %u): both ends have colour %u\n", v, u, lpa.colors()[v]);
        }
        uint32_t best = 0;
        for (std::map<uint32_t, uint32_t>::const_iterator it = cnt.begin(); it != cnt.end(); ++it) best = std::max(best, it->second);
        if (lpa.converged() && cnt[label[v]] < best && bad++ < 5)
            printf("vertex %zu: %u neighbours carry its label %u and %u carry another one\n", v, cnt[label[v]], label[v], best);
    }
    for (size_t c = 0; c < lpa.community_sizes().size(); c++) members += lpa.community_sizes()[c];
    if (members != lpa.num_real_vertices() || lpa.community_labels().size() != lpa.num_communities()) {
        printf("%llu members of %llu communities, %u real vertices\n", members, (unsigned long long)lpa.num_communities(), lpa.num_real_vertices());
        bad++;
    }
    const char *names[2] = {"/cpp_label.bin", "/cpp_color.bin"};
    const std::vector<uint32_t> *words[2] = {&lpa.labels(), &lpa.colors()};
    for (int i = 0; i < 2; i++) {
        const std::string p = out + names[i];
        FILE *f = fopen(p.c_str(), "wb");
        if (!f || fwrite(words[i]->data(), sizeof(uint32_t), words[i]->size(), f) != words[i]->size()) { printf("cannot write %s\n", p.c_str()); return 2; }
        fclose(f);
    }
    printf("sweeps: %llu\nchanges: %llu\nevaluations: %llu\nconverged: %d\ncolours: %llu\ncommunities: %llu\nmodularity: %.17g\nchecksum: %llu\n",
           (unsigned long long)lpa.sweeps(), (unsigned long long)lpa.changes(), (unsigned long long)lpa.evaluations(), lpa.converged() ? 1 : 0,
           (unsigned long long)lpa.num_colors(), (unsigned long long)lpa.num_communities(), lpa.modularity(), checksum);
    if (!bad) printf("LabelPropagation::run OK\n");
    return bad ? 1 : 0;
}
