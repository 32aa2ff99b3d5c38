// graphlily::app::ConnectedComponents driven from C++: the labels are written as raw 32-bit words for tests/test_gpu_cc.py to
// compare with the Python driver's, the count is printed, and rule 1 of app.validate_components is checked here: a label is
// not above its vertex and is its own label.
//   cc_driver graph.npz out_dir
//   g++ -std=c++11 -I<repo>/include tests/cpp/cc_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/cc.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    graphlily::app::ConnectedComponents cc(graphlily::num_hbm_channels, 1024, 256);
    cc.set_target("hw");
    cc.set_up_runtime("unused.xclbin");
    cc.load_and_format_matrix(npz, true);
    cc.send_matrix_host_to_device();
    auto labels = cc.run();
    int bad = 0;
    if (labels.size() != cc.num_vertices()) { printf("size mismatch\n"); return 1; }
    uint32_t roots = 0;
    for (size_t v = 0; v < labels.size() && bad < 5; v++) {
        const uint32_t l = labels[v];
        if (l > v || labels[l] != l) { printf("vertex %zu has label %u, whose label is %u\n", v, l, l < labels.size() ? labels[l] : 0u); bad++; }
        roots += l == v && v < cc.num_real_vertices();
    }
    if (!bad && roots != cc.num_components()) { printf("%u roots among the real vertices, num_components() = %u\n", roots, cc.num_components()); bad++; }
    const std::string p = out + "/cpp_labels.bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(labels.data(), sizeof(labels[0]), labels.size(), f) != labels.size()) { printf("cannot write %s\n", p.c_str()); return 2; }
    fclose(f);
    printf("components: %u\nlargest: %u\n", cc.num_components(), cc.largest_component());
    if (!bad) printf("ConnectedComponents::run OK\n");
    return bad ? 1 : 0;
}
