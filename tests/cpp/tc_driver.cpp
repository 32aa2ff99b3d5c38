// graphlily::app::TriangleCount driven from C++: the per-vertex counts are written as raw 64-bit words for tests/test_gpu_tc.py
// to compare with the Python driver's, the total is printed, and what ties the two outputs together is checked here: every
// triangle has three corners, so the counts add up to three times the total, and a vertex of degree d lies in at most
// d (d - 1) / 2 triangles.
//   tc_driver graph.npz out_dir
//   g++ -std=c++11 -I<repo>/include tests/cpp/tc_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/tc.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    graphlily::app::TriangleCount tc(graphlily::num_hbm_channels, 1024, 256);
    tc.set_target("hw");
    tc.set_up_runtime("unused.xclbin");
    tc.load_and_format_matrix(npz, true);
    tc.send_matrix_host_to_device();
    auto counts = tc.run();
    int bad = 0;
    if (counts.size() != tc.num_vertices() || tc.degrees().size() != counts.size()) { printf("size mismatch\n"); return 1; }
    unsigned long long sum = 0;
    for (size_t v = 0; v < counts.size() && bad < 5; v++) {
        const unsigned long long d = tc.degrees()[v], t = counts[v];
        if (t > d * (d ? d - 1 : 0) / 2) { printf("vertex %zu of degree %llu is given %llu triangles\n", v, d, t); bad++; }
        sum += t;
    }
    if (!bad && sum != 3ull * tc.num_triangles()) { printf("the counts add up to %llu, num_triangles() = %llu\n", sum, (unsigned long long)tc.num_triangles()); bad++; }
    const std::string p = out + "/cpp_triangles.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(counts.data(), sizeof(counts[0]), counts.size(), f) != counts.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("triangles: %llu\ntransitivity: %.17g\n", (unsigned long long)tc.num_triangles(), tc.transitivity());
    if (!bad) printf("TriangleCount::run OK\n");
    return bad ? 1 : 0;
}
