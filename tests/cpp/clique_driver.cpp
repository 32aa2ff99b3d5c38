// graphlily::app::CliqueCount driven from C++: the per-vertex counts are written as raw 64-bit words for tests/test_gpu_clique.py
// to compare with the Python driver's, the total is printed, and what ties the outputs together is checked here: every k-clique
// has k corners, so the counts add up to k times the total, and the total-only kernels give the same total.
//   clique_driver graph.npz out_dir k
//   g++ -std=c++11 -I<repo>/include tests/cpp/clique_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/clique.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 4) { printf("usage: %s graph.npz out_dir k\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const uint32_t k = (uint32_t)atoi(argv[3]);
    graphlily::app::CliqueCount cc(graphlily::num_hbm_channels, 1024, 256);
    cc.set_target("hw");
    cc.set_up_runtime("unused.xclbin");
    cc.load_and_format_matrix(npz, true);
    cc.send_matrix_host_to_device();
    auto counts = cc.run(k);
    if (counts.size() != cc.num_vertices()) { printf("size mismatch\n"); return 1; }
    int bad = 0;
    unsigned long long sum = 0;
    for (size_t v = 0; v < counts.size(); v++) sum += counts[v];
    const unsigned long long total = cc.num_cliques();
    if (sum != (unsigned long long)k * total) { printf("the counts add up to %llu, num_cliques() = %llu\n", sum, total); bad++; }
    if (cc.run_total(k) != total) { printf("the total-only run gives %llu, the per-vertex run %llu\n", (unsigned long long)cc.num_cliques(), total); bad++; }
    const std::string p = out + "/cpp_cliques.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(counts.data(), sizeof(counts[0]), counts.size(), f) != counts.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("k: %u\ncliques: %llu\ndensity: %.17g\n", cc.k(), total, cc.clique_density());
    if (!bad) printf("CliqueCount::run OK\n");
    return bad ? 1 : 0;
}
