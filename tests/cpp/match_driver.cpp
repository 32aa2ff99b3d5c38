// graphlily::app::Matching driven from C++: the mates are written as raw 32-bit words for tests/test_gpu_match.py to compare with
// the Python driver's, the matched edges, rounds, scans, total weight and a checksum are printed, and what ties the outputs
// together is checked here: mate is an involution without fixed points, every pair is an edge of graph(), no edge of graph() has
// two free ends, and edges() lists exactly the pairs, once each, in ascending order.
//   match_driver graph.npz out_dir [weighted: 1 (default) or 0] [drop_nonpositive: 0 (default) or 1]
//   g++ -std=c++11 -I<repo>/include tests/cpp/match_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/matching.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir [weighted] [drop_nonpositive]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const bool weighted = argc < 4 || atoi(argv[3]) != 0, drop = argc > 4 && atoi(argv[4]) != 0;
    graphlily::app::Matching match(graphlily::num_hbm_channels, 1024, 256);
    match.set_target("hw");
    match.set_up_runtime("unused.xclbin");
    match.load_and_format_matrix(npz, true, weighted, drop);
    match.send_matrix_host_to_device();
    auto mate = match.run();
    int bad = 0;
    const size_t n = match.num_vertices();
    const uint32_t kFree = graphlily::app::Matching::kFree;
    if (mate.size() != n || match.mate().size() != n || match.edges().size() != match.num_matched() || match.weights().size() != match.num_matched()) {
        printf("size mismatch\n");
        return 1;
    }
    unsigned long long matched = 0, checksum = 0, listed = 0;
    for (size_t v = 0; v < n; v++) {
        checksum = checksum * 1000003ull + mate[v] + 1ull;          // (mod 2^64: tests/test_gpu_match.py computes the same)
        if (mate[v] == kFree) continue;
        matched++;
        if ((mate[v] >= n || mate[v] == v || mate[mate[v]] != v) && bad++ < 5) printf("vertex %zu is matched to %u, which is not matched to it\n", v, mate[v]);
    }
    const CSRMatrix<float> &g = match.graph();
    for (size_t v = 0; v < n && bad < 5; v++) {
        bool stored = mate[v] == kFree;
        for (uint32_t j = g.adj_indptr[v]; j < g.adj_indptr[v + 1]; j++) {
            const uint32_t u = g.adj_indices[j];
            stored |= u == mate[v];
            if (mate[v] == kFree && mate[u] == kFree && bad++ < 5) printf("both ends of edge (%zu, %u) are free\n", v, u);
        }
        if (!stored && bad++ < 5) printf("vertex %zu is matched to %u over no edge\n", v, mate[v]);
    }
    for (size_t i = 0; i < match.edges().size(); i++) {
        const std::pair<uint32_t, uint32_t> e = match.edges()[i];
        listed += mate[e.first] == e.second;
        if ((e.first >= e.second || (i && !(match.edges()[i - 1] < e))) && bad++ < 5) printf("matched edge %zu (%u, %u) is out of order\n", i, e.first, e.second);
    }
    if (matched != 2 * match.num_matched() || listed != match.num_matched()) {
        printf("%llu matched vertices, %llu listed pairs, num_matched() = %llu\n", matched, listed, (unsigned long long)match.num_matched());
        bad++;
    }
    const std::string p = out + "/cpp_mate.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(mate.data(), sizeof(mate[0]), mate.size(), f) != mate.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("matched edges: %llu\nrounds: %llu\nscans: %llu\ntotal weight: %.17g\nchecksum: %llu\n", (unsigned long long)match.num_matched(),
           (unsigned long long)match.rounds(), (unsigned long long)match.scans(), match.total_weight(), checksum);
    if (!bad) printf("Matching::run OK\n");
    return bad ? 1 : 0;
}
