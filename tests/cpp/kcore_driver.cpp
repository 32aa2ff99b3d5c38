// graphlily::app::KCore driven from C++: the core numbers are written as raw 32-bit words for tests/test_gpu_kcore.py to compare
// with the Python driver's, the degeneracy, the sum of the core numbers and a checksum are printed, and what ties the outputs
// together is checked here: no core number exceeds the degree or the degeneracy, some vertex attains the degeneracy, the order is
// a permutation along which the core numbers never descend, and core_sizes()[0] counts every real vertex.
//   kcore_driver graph.npz out_dir            run on the device
//   kcore_driver --symmetrize graph.npz       host only: print graphlily::io::util_symmetrize_simple's result after padding
//   g++ -std=c++11 -I<repo>/include tests/cpp/kcore_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/kcore.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir | --symmetrize graph.npz\n", argv[0]); return 2; }
    if (std::string(argv[1]) == "--symmetrize") {
        CSRMatrix<float> m = graphlily::io::load_csr_matrix_from_float_npz(argv[2]);
        graphlily::io::util_round_csr_matrix_dim(m, 128, 128);
        std::vector<uint32_t> deg;
        CSRMatrix<float> s = graphlily::io::util_symmetrize_simple(m, deg);
        printf("shape: %u %u\nindptr:", s.num_rows, s.num_cols);
        for (uint32_t x : s.adj_indptr) printf(" %u", x);
        printf("\nindices:");
        for (uint32_t x : s.adj_indices) printf(" %u", x);
        printf("\ndata:");
        for (float x : s.adj_data) printf(" %g", x);
        printf("\ndegrees:");
        for (uint32_t x : deg) printf(" %u", x);
        printf("\n");
        return 0;
    }
    const std::string npz = argv[1], out = argv[2];
    graphlily::app::KCore kc(graphlily::num_hbm_channels, 1024, 256);
    kc.set_target("hw");
    kc.set_up_runtime("unused.xclbin");
    kc.load_and_format_matrix(npz, true);
    kc.send_matrix_host_to_device();
    auto core = kc.run(true);
    int bad = 0;
    const size_t n = kc.num_vertices();
    if (core.size() != n || kc.degrees().size() != n || kc.order().size() != n) { printf("size mismatch\n"); return 1; }
    unsigned long long sum = 0, checksum = 0;
    uint32_t top = 0;
    for (size_t v = 0; v < n; v++) {
        if ((core[v] > kc.degrees()[v] || core[v] > kc.degeneracy()) && bad++ < 5)
            printf("vertex %zu of degree %u is given core number %u (degeneracy %u)\n", v, kc.degrees()[v], core[v], kc.degeneracy());
        top = core[v] > top ? core[v] : top;
        sum += core[v];
        checksum = checksum * 1000003ull + core[v] + 1ull;        // (mod 2^64: tests/test_gpu_kcore.py computes the same)
    }
    if (top != kc.degeneracy()) { printf("the largest core number is %u, degeneracy() = %u\n", top, kc.degeneracy()); bad++; }
    std::vector<unsigned char> seen(n, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = kc.order()[i];
        if ((v >= n || seen[v]++) && bad++ < 5) printf("order[%zu] = %u: not a permutation\n", i, v);
        else if (i && v < n && kc.order()[i - 1] < n && core[kc.order()[i - 1]] > core[v] && bad++ < 5) printf("order[%zu]: the core numbers descend\n", i);
    }
    if (kc.core_sizes().size() != (size_t)kc.degeneracy() + 1 || kc.core_sizes()[0] != kc.num_real_vertices()) { printf("core_sizes() is off\n"); bad++; }
    const std::string p = out + "/cpp_core.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(core.data(), sizeof(core[0]), core.size(), f) != core.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("degeneracy: %u\nsum of core numbers: %llu\nchecksum: %llu\nlevels: %u\nsub-rounds: %u\n", kc.degeneracy(), sum, checksum, kc.levels(),
           kc.sub_rounds());
    if (!bad) printf("KCore::run OK\n");
    return bad ? 1 : 0;
}
