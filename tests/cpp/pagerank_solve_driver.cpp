// graphlily::app::PageRank::solve() driven from C++: personalised PageRank with dangling mass and a residual stop (DESIGN.md
// 4.11).  Without seed vertices the teleport is uniform over the matrix's own vertices; with them it is uniform over the seeds.
// The ranks (32-bit words) and the residual history (64-bit words) are written raw for tests/test_gpu_pagerank_solve.py to
// compare with the Python driver's, and what needs no reference is checked here: one residual per iteration, the last one
// <= tol exactly if the run converged, padding at 0, the ranks summing to 1, and pull() returning after the solve the words
// it returned before it (solve leaves the module's bindings as it found them).
//   pagerank_solve_driver graph.npz out_dir damping tol max_iterations [seed vertices...]
//   g++ -std=c++11 -I<repo>/include tests/cpp/pagerank_solve_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/pagerank.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (argc < 6) { printf("usage: %s graph.npz out_dir damping tol max_iterations [seed vertices...]\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    const float damping = (float)atof(argv[3]);
    const double tol = atof(argv[4]);
    const uint32_t max_iterations = (uint32_t)atoi(argv[5]);
    graphlily::app::PageRank pagerank(graphlily::num_hbm_channels, 1024, 256);
    pagerank.set_target("hw");
    pagerank.set_up_runtime("unused.xclbin");
    pagerank.load_and_format_matrix(npz, damping, true);
    pagerank.send_matrix_host_to_device();
    const uint32_t n0 = graphlily::io::load_csr_matrix_from_float_npz(npz).num_rows;
    std::vector<float> p;
    if (argc > 6) {
        p.assign(n0, 0.0f);
        for (int i = 6; i < argc; i++) {
            const uint32_t v = (uint32_t)atoi(argv[i]);
            if (v >= n0) { printf("seed %u of %u vertices\n", v, n0); return 2; }
            p[v] = 1.0f;
        }
    }
    const auto pulled = pagerank.pull(damping, 3);
    auto rank = pagerank.solve(damping, tol, max_iterations, p);
    const std::vector<double> &r = pagerank.residuals();
    int bad = 0;
    if (r.size() != pagerank.iterations() || r.empty() || r.size() > max_iterations) {
        printf("%zu residuals for %u iterations of at most %u\n", r.size(), pagerank.iterations(), max_iterations);
        bad++;
    }
    for (size_t k = 0; k < r.size() && !bad; k++) {
        const bool last = k + 1 == r.size();
        if ((r[k] <= tol) != (last && pagerank.converged())) {
            printf("residual %zu of %zu is %g with tol %g, converged() says %d\n", k + 1, r.size(), r[k], tol, (int)pagerank.converged());
            bad++;
        }
    }
    if (!pagerank.converged() && pagerank.iterations() != max_iterations) {
        printf("stopped after %u of %u iterations without converging\n", pagerank.iterations(), max_iterations);
        bad++;
    }
    double sum = 0;
    for (size_t v = 0; v < rank.size(); v++) {
        sum += (double)rank[v];
        if (v >= n0 && rank[v] != 0.0f) { printf("padding vertex %zu has rank %g\n", v, rank[v]); bad++; break; }
    }
    if (!(std::fabs(sum - 1.0) <= 1e-6)) { printf("the ranks sum to %.9f\n", sum); bad++; }
    const auto again = pagerank.pull(damping, 3);
    if (again.size() != pulled.size() || memcmp(again.data(), pulled.data(), sizeof(pulled[0]) * pulled.size()) != 0) {
        printf("pull() after solve() differs from pull() before it\n");
        bad++;
    }
    dump(out, "cpp_ranks", rank);
    dump(out, "cpp_residuals", r);
    printf("iterations %u converged %d\n", pagerank.iterations(), (int)pagerank.converged());
    if (!bad) printf("PageRank::solve OK\n");
    return bad ? 1 : 0;
}
