// graphlily::app::Louvain driven from C++: the labels are written as raw 32-bit words for tests/test_gpu_louvain.py to compare with
// the Python driver's, the per-level statistics, the communities, the modularity and a checksum are printed, and what ties the
// outputs together is checked here: every vertex carries the smallest vertex of its community, an isolated vertex its own number,
// the community sizes add up to the real vertices, the last accepted level's Q over two_m^2 is the modularity, and the dendrogram's
// last level induces the labels.
//   louvain_driver graph.npz out_dir [order: largest_first (default), natural, random, smallest_last] [seed: 0] [max_sweeps: 100]
//                  [max_levels: 32] [tol: 1e-7]
//   g++ -std=c++11 -I<repo>/include tests/cpp/louvain_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/louvain.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir [order] [seed] [max_sweeps] [max_levels] [tol]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2], order = argc > 3 ? argv[3] : "largest_first";
    const long seed = argc > 4 ? atol(argv[4]) : 0, max_sweeps = argc > 5 ? atol(argv[5]) : 100, max_levels = argc > 6 ? atol(argv[6]) : 32;
    const double tol = argc > 7 ? atof(argv[7]) : 1e-7;
    graphlily::app::Louvain lv(graphlily::num_hbm_channels, 1024, 256);
    lv.set_target("hw");
    lv.set_up_runtime("unused.xclbin");
    lv.load_and_format_matrix(npz, true);
    lv.send_matrix_host_to_device();
    auto label = lv.run(tol, (uint32_t)max_sweeps, (uint32_t)max_levels, order, (uint32_t)seed);
    int bad = 0;
    const size_t n = lv.num_vertices();
    if (label.size() != n || lv.labels().size() != n) {
        printf("size mismatch\n");
        return 1;
    }
    const CSRMatrix<float> &g = lv.graph();
    unsigned long long checksum = 0, members = 0;
    for (size_t v = 0; v < n; v++) {
        checksum = checksum * 1000003ull + label[v] + 1ull;          // (mod 2^64: tests/test_gpu_louvain.py computes the same)
        if ((label[v] > v || label[label[v]] != label[v]) && bad++ < 5) printf("vertex %zu carries %u, not the smallest vertex of a community\n", v, label[v]);
        if (g.adj_indptr[v] == g.adj_indptr[v + 1] && label[v] != v && bad++ < 5) printf("vertex %zu has no neighbour and carries %u\n", v, label[v]);
    }
    for (size_t c = 0; c < lv.community_sizes().size(); c++) members += lv.community_sizes()[c];
    if (members != lv.num_real_vertices() || lv.community_labels().size() != lv.num_communities()) {
        printf("%llu members of %llu communities, %u real vertices\n", members, (unsigned long long)lv.num_communities(), lv.num_real_vertices());
        bad++;
    }
    const size_t runs = lv.level_sizes().size();
    if (lv.levels() > runs || runs > lv.levels() + 1 || lv.dendrogram().size() != lv.levels() || lv.level_q().size() != runs) {
        printf("%llu accepted levels of %zu runs\n", (unsigned long long)lv.levels(), runs);
        bad++;
    }
    if (lv.levels()) {
        const std::vector<uint32_t> &last = lv.dendrogram().back();
        for (size_t v = 0; v < n; v++)
            if ((last[v] == last[label[v]]) != true && bad++ < 5) printf("vertex %zu and its label %u are in different communities of the last level\n", v, label[v]);
        const double two_m = (double)g.adj_indices.size();
        const double q = (double)lv.level_q()[lv.levels() - 1].second / (two_m * two_m);
        if (std::fabs(q - lv.modularity()) > 1e-9 && bad++ < 5) printf("Q / two_m^2 = %.12f, modularity %.12f\n", q, lv.modularity());
    }
    const std::string p = out + "/cpp_label.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(lv.labels().data(), sizeof(uint32_t), n, f) != n) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("levels: %llu\nlaunches: %llu\ncommunities: %llu\nmodularity: %.17g\nchecksum: %llu\n", (unsigned long long)lv.levels(),
           (unsigned long long)lv.launches(), (unsigned long long)lv.num_communities(), lv.modularity(), checksum);
    for (size_t i = 0; i < runs; i++)
        printf("level %zu: size %llu colours %llu sweeps %llu moves %llu q_first %lld q_last %lld\n", i, (unsigned long long)lv.level_sizes()[i],
               (unsigned long long)lv.level_colors()[i], (unsigned long long)lv.level_sweeps()[i], (unsigned long long)lv.level_moves()[i],
               (long long)lv.level_q()[i].first, (long long)lv.level_q()[i].second);
    if (!bad) printf("Louvain::run OK\n");
    return bad ? 1 : 0;
}
