// graphlily::app::KTruss driven from C++: the truss numbers and the supports are written as raw 32-bit words for
// tests/test_gpu_truss.py to compare with the Python driver's, the largest truss number, the sum over the edges, the triangles and
// a checksum are printed, and what ties the outputs together is checked here: every entry has a truss number between 2 and
// max_truss() that is at most its support + 2, some entry attains max_truss(), the supports add up to three per triangle, and
// truss_sizes()[0] counts every edge.
//   truss_driver graph.npz out_dir
//   g++ -std=c++11 -I<repo>/include tests/cpp/truss_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/truss.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    graphlily::app::KTruss kt(graphlily::num_hbm_channels, 1024, 256);
    kt.set_target("hw");
    kt.set_up_runtime("unused.xclbin");
    kt.load_and_format_matrix(npz, true);
    kt.send_matrix_host_to_device();
    auto truss = kt.run(true);
    int bad = 0;
    const size_t nnz = kt.graph().adj_indices.size();
    if (truss.size() != nnz || kt.support().size() != nnz || kt.vertex_truss().size() != kt.num_vertices()) { printf("size mismatch\n"); return 1; }
    unsigned long long sum = 0, checksum = 0, support_sum = 0;
    uint32_t top = 0;
    for (size_t j = 0; j < nnz; j++) {
        if ((truss[j] < 2 || truss[j] > kt.max_truss() || truss[j] > kt.support()[j] + 2) && bad++ < 5)
            printf("entry %zu with support %u is given truss %u (max_truss %llu)\n", j, kt.support()[j], truss[j], (unsigned long long)kt.max_truss());
        top = truss[j] > top ? truss[j] : top;
        sum += truss[j];
        support_sum += kt.support()[j];
        checksum = checksum * 1000003ull + truss[j] + 1ull;        // (mod 2^64: tests/test_gpu_truss.py computes the same)
    }
    if (top != kt.max_truss()) { printf("the largest truss number is %u, max_truss() = %llu\n", top, (unsigned long long)kt.max_truss()); bad++; }
    if (2 * kt.num_edges() != nnz) { printf("num_edges() = %llu for %zu entries\n", (unsigned long long)kt.num_edges(), nnz); bad++; }
    if (support_sum != 6 * kt.num_triangles()) { printf("the supports add up to %llu, num_triangles() = %llu\n", support_sum, (unsigned long long)kt.num_triangles()); bad++; }
    if (kt.truss_sizes().size() != (size_t)kt.max_truss() + 1 || kt.truss_sizes()[0] != kt.num_edges()) { printf("truss_sizes() is off\n"); bad++; }
    const std::string p = out + "/cpp_truss.bin", q = out + "/cpp_support.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(truss.data(), sizeof(truss[0]), truss.size(), f) != truss.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    f = fopen(q.c_str(), "wb");
    if (!f || fwrite(kt.support().data(), sizeof(uint32_t), nnz, f) != nnz) { printf("cannot write %s\n", q.c_str()); return 2; }
    fclose(f);
    printf("max truss: %llu\nsum of truss over edges: %llu\ntriangles: %llu\nchecksum: %llu\nlevels: %llu\nsub-rounds: %llu\n",
           (unsigned long long)kt.max_truss(), sum / 2, (unsigned long long)kt.num_triangles(), checksum, (unsigned long long)kt.levels(),
           (unsigned long long)kt.sub_rounds());
    if (!bad) printf("KTruss::run OK\n");
    return bad ? 1 : 0;
}
