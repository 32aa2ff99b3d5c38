// graphlily::app::GraphColoring driven from C++: the colours are written as raw 32-bit words for tests/test_gpu_coloring.py to
// compare with the Python driver's, the number of colours, the rounds, the widest round, the sum of the colours and a checksum are
// printed, and what ties the outputs together is checked here: no colour exceeds the degree or reaches num_colors(), some vertex
// attains num_colors() - 1, no stored entry joins two vertices of one colour, and color_sizes() counts every real vertex.
//   coloring_driver graph.npz out_dir order seed          run on the device (order: natural | random | largest_first | smallest_last)
//   coloring_driver --priorities graph.npz order seed     host only: print graphlily::io::util_coloring_priorities after padding
//   g++ -std=c++11 -I<repo>/include tests/cpp/coloring_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/coloring.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 5) { printf("usage: %s graph.npz out_dir order seed | --priorities graph.npz order seed\n", argv[0]); return 2; }
    const std::string order = argv[3];
    const uint32_t seed = (uint32_t)strtoul(argv[4], nullptr, 10);
    if (std::string(argv[1]) == "--priorities") {
        CSRMatrix<float> m = graphlily::io::load_csr_matrix_from_float_npz(argv[2]);
        graphlily::io::util_round_csr_matrix_dim(m, 128, 128);
        std::vector<uint32_t> deg;
        CSRMatrix<float> s = graphlily::io::util_symmetrize_simple(m, deg);
        std::vector<uint32_t> prio = graphlily::io::util_coloring_priorities(deg, order, seed);
        printf("vertices: %u\npriorities:", s.num_rows);
        for (uint32_t x : prio) printf(" %u", x);
        printf("\n");
        return 0;
    }
    const std::string npz = argv[1], out = argv[2];
    graphlily::app::GraphColoring gc(graphlily::num_hbm_channels, 1024, 256);
    gc.set_target("hw");
    gc.set_up_runtime("unused.xclbin");
    gc.load_and_format_matrix(npz, true);
    gc.send_matrix_host_to_device();
    auto color = gc.run(order, seed);
    int bad = 0;
    const size_t n = gc.num_vertices();
    if (color.size() != n || gc.degrees().size() != n || (order != "natural" && gc.priorities().size() != n)) { printf("size mismatch\n"); return 1; }
    unsigned long long sum = 0, checksum = 0;
    uint32_t top = 0;
    for (size_t v = 0; v < n; v++) {
        if ((color[v] > gc.degrees()[v] || color[v] >= gc.num_colors()) && bad++ < 5)
            printf("vertex %zu of degree %u is given colour %u (%llu colours)\n", v, gc.degrees()[v], color[v], (unsigned long long)gc.num_colors());
        top = color[v] > top ? color[v] : top;
        sum += color[v];
        checksum = checksum * 1000003ull + color[v] + 1ull;       // (mod 2^64: tests/test_gpu_coloring.py computes the same)
    }
    if ((unsigned long long)top + 1ull != gc.num_colors()) { printf("the largest colour is %u, num_colors() = %llu\n", top, (unsigned long long)gc.num_colors()); bad++; }
    // the edges as the driver stored them: the matrix prepared again on the host
    {
        CSRMatrix<float> m = graphlily::io::load_csr_matrix_from_float_npz(npz);
        graphlily::io::util_round_csr_matrix_dim(m, graphlily::num_hbm_channels * graphlily::pack_size, graphlily::num_hbm_channels * graphlily::pack_size);
        std::vector<uint32_t> deg;
        CSRMatrix<float> s = graphlily::io::util_symmetrize_simple(m, deg);
        for (uint32_t v = 0; v < s.num_rows && v < n; v++)
            for (uint32_t i = s.adj_indptr[v]; i < s.adj_indptr[v + 1]; i++)
                if (s.adj_indices[i] < n && color[s.adj_indices[i]] == color[v] && bad++ < 5)
                    printf("the neighbours %u and %u both have colour %u\n", v, s.adj_indices[i], color[v]);
    }
    unsigned long long counted = 0;
    for (uint64_t c : gc.color_sizes()) counted += c;
    if (gc.color_sizes().size() != gc.num_colors() || counted != gc.num_real_vertices()) { printf("color_sizes() is off\n"); bad++; }
    if (order == "smallest_last" && gc.num_colors() > (unsigned long long)gc.degeneracy() + 1ull) {
        printf("%llu colours, degeneracy %u\n", (unsigned long long)gc.num_colors(), gc.degeneracy());
        bad++;
    }
    const std::string p = out + "/cpp_color.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(color.data(), sizeof(color[0]), color.size(), f) != color.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("colours: %llu\nrounds: %llu\nwidest: %llu\nsum of colours: %llu\nchecksum: %llu\n", (unsigned long long)gc.num_colors(),
           (unsigned long long)gc.rounds(), (unsigned long long)gc.widest(), sum, checksum);
    if (!bad) printf("GraphColoring::run OK\n");
    return bad ? 1 : 0;
}
