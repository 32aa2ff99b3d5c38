// graphlily::app::BFS::parents() driven from C++: pull_push on the device-resident schedule, then the predecessor tree from the
// levels still on the device (gl_bfs_parents), and the same from the host vector the search returned.  Levels and parents are
// written as raw 32-bit words for tests/test_gpu_bfs_parents.py to compare with the Python driver's, and checked here against
// the definition on the class's own compute_reference_results: the source is its own parent, an unreached vertex has none, every
// other parent sits one level up.
//   bfs_parents_driver graph.npz out_dir source iterations
//   g++ -std=c++11 -I<repo>/include tests/cpp/bfs_parents_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/bfs.h"

#include <cstdio>
#include <cstdlib>
#include <string>

template <typename V>
static void dump(const std::string &dir, const char *name, const V &v) {
    const std::string p = dir + "/" + name + ".bin";
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(v.data(), sizeof(v[0]), v.size(), f) != v.size()) {
        printf("cannot write %s\n", p.c_str());
        exit(2);
    }
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc < 5) { printf("usage: %s graph.npz out_dir source iterations\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const uint32_t source = (uint32_t)atoi(argv[3]), iters = (uint32_t)atoi(argv[4]);
    graphlily::app::BFS bfs(graphlily::num_hbm_channels, 1024, 512, 256);
    bfs.set_target("hw");
    bfs.set_up_runtime("unused.xclbin");
    bfs.load_and_format_matrix(npz, true);
    bfs.send_matrix_host_to_device();
    auto levels = bfs.pull_push(source, iters);
    auto parent = bfs.parents();
    const uint32_t orphans = bfs.orphans();
    auto again = bfs.parents(levels);
    int bad = 0;
    if (parent.size() != levels.size() || again.size() != levels.size()) { printf("size mismatch\n"); return 1; }
    if (orphans != 0 || bfs.orphans() != 0) { printf("%u / %u orphans in a BFS result\n", orphans, bfs.orphans()); bad++; }
    auto ref = bfs.compute_reference_results(source, iters);
    for (size_t v = 0; v < levels.size() && bad < 5; v++) {
        const float d = ref[v];
        const uint32_t p = parent[v];
        if (float(levels[v]) != d) { printf("level mismatch at %zu\n", v); bad++; }
        if (again[v] != p) { printf("parents(levels) differs from parents() at %zu: %u vs %u\n", v, again[v], p); bad++; }
        if (d == 0.0f ? p != 0xffffffffu : d == 1.0f ? p != v : (p >= levels.size() || ref[p] != d - 1.0f)) {
            printf("vertex %zu on level %g has parent %u\n", v, d, p);
            bad++;
        }
    }
    dump(out, "cpp_levels", levels);
    dump(out, "cpp_parents", parent);
    if (!bad) printf("BFS::parents OK\n");
    return bad ? 1 : 0;
}
