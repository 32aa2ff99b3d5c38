// graphlily::app::SSSP::parents() driven from C++: weighted pull_push (the matrix's own weights, a weight-0 diagonal per row),
// then the predecessor tree from the distances still on the device (gl_sssp_parents), and the same from the host vector the
// search returned.  Distances and parents are written as raw 32-bit words for tests/test_gpu_sssp_parents.py to compare with
// the Python driver's, and rules 1-3 of the tree are checked here: the source has distance 0 and is its own parent, a vertex is
// reached exactly if it has a parent, and every other parent is strictly nearer and joined by a stored entry whose weight makes
// up the difference in float arithmetic.
//   sssp_parents_driver graph.npz out_dir source iterations
//   g++ -std=c++11 -I<repo>/include tests/cpp/sssp_parents_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/sssp.h"

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
    graphlily::app::SSSP sssp(graphlily::num_hbm_channels, 1024, 512, 256);
    sssp.set_target("hw");
    sssp.set_up_runtime("unused.xclbin");
    sssp.load_and_format_matrix(npz, true, true);
    sssp.send_matrix_host_to_device();
    auto distance = sssp.pull_push(source, iters);
    auto parent = sssp.parents();
    const uint32_t orphans = sssp.orphans();
    auto again = sssp.parents(distance, source);
    if (parent.size() != distance.size() || again.size() != distance.size()) { printf("size mismatch\n"); return 1; }
    int bad = 0;
    if (orphans != sssp.orphans()) { printf("%u orphans, then %u\n", orphans, sssp.orphans()); bad++; }
    // the prepared matrix once more, as the class prepared it: rule 3 needs its entries
    graphlily::io::CSRMatrix<float> m = graphlily::io::load_csr_matrix_from_float_npz(npz);
    graphlily::app::detail::sssp_zero_diagonal(m);
    const float unreached = graphlily::TropicalSemiring.zero;
    const size_t n = distance.size();
    if (float(distance[source]) != 0.0f || parent[source] != source) {
        printf("source %u has distance %g and parent %u (rule 1)\n", source, float(distance[source]), parent[source]);
        bad++;
    }
    uint32_t without = 0;
    for (size_t v = 0; v < n && bad < 5; v++) {
        const float d = distance[v];
        const uint32_t p = parent[v];
        if (again[v] != p) { printf("parents(distance, source) differs from parents() at %zu: %u vs %u\n", v, again[v], p); bad++; }
        if (v == source) continue;
        if (!(d < unreached)) {
            if (p != 0xffffffffu) { printf("unreached vertex %zu has parent %u (rule 2)\n", v, p); bad++; }
            continue;
        }
        if (p == 0xffffffffu) { without++; continue; }
        bool tight = false;
        if (p < n && v < m.num_rows && float(distance[p]) < d)
            for (uint32_t i = m.adj_indptr[v]; i < m.adj_indptr[v + 1] && !tight; i++)
                tight = m.adj_indices[i] == p && float(distance[p]) + m.adj_data[i] == d;
        if (!tight) { printf("vertex %zu at distance %g has parent %u (rule 3)\n", v, d, p); bad++; }
    }
    if (without != orphans) { printf("%u reached vertices without a parent, orphans() says %u (rule 2)\n", without, orphans); bad++; }
    dump(out, "cpp_distance", distance);
    dump(out, "cpp_parents", parent);
    if (!bad) printf("SSSP::parents OK (%u orphans)\n", orphans);
    return bad ? 1 : 0;
}
