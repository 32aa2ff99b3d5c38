// graphlily::app::MinimumSpanningForest driven from C++: the forest words and the labels are written as raw 32-bit words for
// tests/test_gpu_msf.py to compare with the Python driver's, the edges, components, rounds, total weight and a checksum are printed,
// and what ties the outputs together is checked here: every word is 0 or 1, edges() lists exactly the marked entries above the
// diagonal in ascending order, both entries of an edge agree in number (the marks add up to twice num_edges()), every forest edge
// joins two vertices of one label, and the roots among the labels number num_components() plus the padding vertices.
//   msf_driver graph.npz out_dir [weighted: 1 (default) or 0]
//   g++ -std=c++11 -I<repo>/include tests/cpp/msf_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/msf.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir [weighted]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const bool weighted = argc < 4 || atoi(argv[3]) != 0;
    graphlily::app::MinimumSpanningForest msf(graphlily::num_hbm_channels, 1024, 256);
    msf.set_target("hw");
    msf.set_up_runtime("unused.xclbin");
    msf.load_and_format_matrix(npz, true, weighted);
    msf.send_matrix_host_to_device();
    auto forest = msf.run(true);
    int bad = 0;
    const size_t nnz = msf.graph().adj_indices.size(), n = msf.num_vertices();
    if (forest.size() != nnz || msf.labels().size() != n || msf.edges().size() != msf.num_edges() || msf.weights().size() != msf.num_edges()) {
        printf("size mismatch\n");
        return 1;
    }
    unsigned long long marks = 0, checksum = 0, roots = 0;
    for (size_t j = 0; j < nnz; j++) {
        if (forest[j] > 1u && bad++ < 5) printf("entry %zu is given %u\n", j, forest[j]);
        marks += forest[j];
        checksum = checksum * 1000003ull + forest[j] + 1ull;        // (mod 2^64: tests/test_gpu_msf.py computes the same)
    }
    for (size_t v = 0; v < n; v++) roots += msf.labels()[v] == v;
    for (size_t i = 0; i < msf.edges().size(); i++) {
        const std::pair<uint32_t, uint32_t> e = msf.edges()[i];
        if ((e.first >= e.second || (i && !(msf.edges()[i - 1] < e)) || msf.labels()[e.first] != msf.labels()[e.second]) && bad++ < 5)
            printf("forest edge %zu (%u, %u) is out of order or joins two labels\n", i, e.first, e.second);
    }
    if (marks != 2 * msf.num_edges()) { printf("%llu marked entries, num_edges() = %llu\n", marks, (unsigned long long)msf.num_edges()); bad++; }
    if (roots != msf.num_components() + (n - msf.num_real_vertices())) { printf("%llu roots among the labels, num_components() = %llu\n", roots, (unsigned long long)msf.num_components()); bad++; }
    if (msf.num_edges() + roots != n) { printf("edges + components != vertices\n"); bad++; }
    const std::string p = out + "/cpp_forest.bin", q = out + "/cpp_labels.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(forest.data(), sizeof(forest[0]), forest.size(), f) != forest.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    f = fopen(q.c_str(), "wb");
    if (!f || fwrite(msf.labels().data(), sizeof(uint32_t), n, f) != n) { printf("cannot write %s\n", q.c_str()); return 2; }
    fclose(f);
    printf("forest edges: %llu\ncomponents: %llu\nrounds: %llu\ntotal weight: %.17g\nchecksum: %llu\n", (unsigned long long)msf.num_edges(),
           (unsigned long long)msf.num_components(), (unsigned long long)msf.rounds(), msf.total_weight(), checksum);
    if (!bad) printf("MinimumSpanningForest::run OK\n");
    return bad ? 1 : 0;
}
