// graphlily::module::SDDMMModule driven from C++: one small rectangular matrix (rows of 0, 1, 5, 70 and 300 entries, so that
// the default cut sends rows to the short and the piece path; an entry stored twice), k = 7 and k = 70, under the three
// semirings, scaled by A's values and not, against the module's own host loop in f64 (compute_reference_results).
//   sddmm_driver
//   g++ -std=c++11 -I<repo>/include tests/cpp/sddmm_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/module/sddmm_module.h"

#include <cmath>
#include <cstdio>
#include <vector>

int main() {
    const uint32_t n = 37, nc = 53;
    const uint32_t lens[5] = {0, 1, 5, 70, 300};
    CSRMatrix<float> a;
    a.num_rows = n;
    a.num_cols = nc;
    a.adj_indptr.push_back(0);
    uint32_t seed = 12345;
    for (uint32_t r = 0; r < n; r++) {
        for (uint32_t e = 0; e < lens[r % 5]; e++) {
            seed = seed * 1664525u + 1013904223u;
            a.adj_indices.push_back((seed >> 8) % nc);
            a.adj_data.push_back((float)((int)((seed >> 20) % 33u) - 16) / 4.0f);
        }
        a.adj_indptr.push_back((uint32_t)a.adj_indices.size());
    }
    graphlily::module::SDDMMModule mm;
    mm.set_target("hw");
    mm.set_up_runtime("unused.xclbin");
    mm.load_and_format_matrix(a);
    mm.send_matrix_host_to_device();
    const graphlily::SemiringType semirings[3] = {graphlily::ArithmeticSemiring, graphlily::LogicalSemiring, graphlily::TropicalSemiring};
    const char *names[3] = {"muladd", "andor", "addmin"};
    const uint32_t ks[2] = {7, 70};
    int bad = 0;
    for (int ki = 0; ki < 2; ki++) {
        const uint32_t k = ks[ki];
        std::vector<float> x((size_t)n * k), y((size_t)nc * k);
        for (size_t i = 0; i < x.size(); i++) x[i] = i % 5 == 0 ? 0.0f : (float)((int)(i * 7 % 23) - 11) / 8.0f;
        for (size_t i = 0; i < y.size(); i++) y[i] = i % 3 == 0 ? 0.0f : (float)((int)(i * 5 % 19) - 9) / 16.0f;
        mm.send_features_host_to_device(x, y, k);
        for (int s = 0; s < 3; s++)
            for (int scaled = 0; scaled < 2; scaled++) {
                mm.set_semiring(semirings[s]);
                mm.set_scaled(scaled != 0);
                mm.run();
                const CSRMatrix<float> c = mm.send_results_device_to_host();
                const std::vector<float> ref = mm.compute_reference_results(x, y, k);
                int wrong = c.adj_data.size() != ref.size() || c.adj_indptr != a.adj_indptr || c.adj_indices != a.adj_indices;
                for (size_t e = 0; e < ref.size() && !wrong; e++) {
                    // x, y and a are small dyadic rationals: the f64 sums are exact in any order, so (+,x) is compared exactly too
                    if (c.adj_data[e] != ref[e]) {
                        printf("%s scaled %d k %u: out[%zu] is %g, expected %g\n", names[s], scaled, k, e, c.adj_data[e], ref[e]);
                        wrong = 1;
                    }
                }
                printf("%s scaled %d k %u: short rows %llu pieces %llu tiles %llu, %s\n", names[s], scaled, k, (unsigned long long)mm.stats()[0],
                       (unsigned long long)mm.stats()[1], (unsigned long long)mm.stats()[2], wrong ? "WRONG" : "ok");
                bad |= wrong;
            }
    }
    if (!bad) printf("ALL CHECKS PASSED\n");
    return bad;
}
