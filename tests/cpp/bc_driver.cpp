// graphlily::app::BetweennessCentrality driven from C++: the values are written as raw doubles for tests/test_gpu_bc.py to compare
// with the Python driver's bit for bit; the depth and the reached count of every search are printed, and what ties the outputs
// together is checked here: every value is finite and >= 0, sources that reach nobody else and padding vertices aside from the
// sums hold 0, no search reports an orphan.
//   bc_driver graph.npz out_dir s0 s1 ...        run the searches from s0, s1, ... on the device
//   bc_driver --pattern graph.npz out_dir        host only: write graphlily::io::util_simple_pattern's result after padding
//   g++ -std=c++11 -I<repo>/include tests/cpp/bc_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/bc.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

static bool write_words(const std::string &path, const void *p, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(p, 1, bytes, f) == bytes;
    if (f) fclose(f);
    if (!ok) printf("cannot write %s\n", path.c_str());
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 4) { printf("usage: %s graph.npz out_dir source... | --pattern graph.npz out_dir\n", argv[0]); return 2; }
    if (std::string(argv[1]) == "--pattern") {
        CSRMatrix<float> m = graphlily::io::load_csr_matrix_from_float_npz(argv[2]), in, out;
        graphlily::io::util_round_csr_matrix_dim(m, 128, 128);
        const bool symmetric = graphlily::io::util_simple_pattern(m, in, out);
        const std::string dir = argv[3];
        printf("symmetric: %d\nshape: %u %u\n", (int)symmetric, in.num_rows, in.num_cols);
        bool ok = write_words(dir + "/cpp_in_indptr.bin", in.adj_indptr.data(), 4 * in.adj_indptr.size()) &&
                  write_words(dir + "/cpp_in_indices.bin", in.adj_indices.data(), 4 * in.adj_indices.size());
        if (!symmetric)
            ok = ok && write_words(dir + "/cpp_out_indptr.bin", out.adj_indptr.data(), 4 * out.adj_indptr.size()) &&
                 write_words(dir + "/cpp_out_indices.bin", out.adj_indices.data(), 4 * out.adj_indices.size());
        return ok ? 0 : 2;
    }
    const std::string npz = argv[1], out = argv[2];
    std::vector<uint32_t> sources;
    for (int i = 3; i < argc; i++) sources.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
    graphlily::app::BetweennessCentrality bc(graphlily::num_hbm_channels, 1024, 512, 256);
    bc.set_target("hw");
    bc.set_up_runtime("unused.xclbin");
    bc.load_and_format_matrix(npz, true);
    bc.send_matrix_host_to_device();
    auto got = bc.run(sources);
    int bad = 0;
    const size_t n = bc.num_vertices();
    if (got.size() != n || bc.depths().size() != sources.size() || bc.reached().size() != sources.size()) { printf("size mismatch\n"); return 1; }
    double sum = 0;
    for (size_t v = 0; v < n; v++) {
        if ((!std::isfinite(got[v]) || got[v] < 0 || (v >= bc.num_real_vertices() && got[v] != 0)) && bad++ < 5)
            printf("vertex %zu is given %g\n", v, got[v]);
        sum += got[v];
    }
    if (bc.orphans() != 0) { printf("%u orphans in BFS results\n", bc.orphans()); bad++; }
    if (!write_words(out + "/cpp_bc.bin", got.data(), sizeof(double) * got.size())) return 2;
    printf("directed: %d\nsum: %.17g\ndepths:", (int)bc.directed(), sum);
    for (uint32_t d : bc.depths()) printf(" %u", d);
    printf("\nreached:");
    for (uint32_t r : bc.reached()) printf(" %u", r);
    printf("\noverflowed: %zu\n", bc.overflowed().size());
    if (!bad) printf("BetweennessCentrality::run OK\n");
    return bad ? 1 : 0;
}
