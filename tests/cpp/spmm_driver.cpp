// graphlily::module::SpMMModule driven from C++: one small rectangular matrix (rows of 0, 1, 5, 70 and 300 entries, so that the
// default cuts send rows to the short and the wavefront path; an entry stored twice; a zero value), k = 7, under the three
// semirings without a mask and with both mask types, against a plain host loop in f64.
//   spmm_driver
//   g++ -std=c++11 -I<repo>/include tests/cpp/spmm_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/module/spmm_module.h"

#include <cmath>
#include <cstdio>
#include <vector>

int main() {
    const uint32_t n = 37, nc = 53, k = 7;
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
            a.adj_data.push_back(e == 3 ? 0.0f : (float)((int)((seed >> 20) % 33u) - 16) / 4.0f);
        }
        a.adj_indptr.push_back((uint32_t)a.adj_indices.size());
    }
    std::vector<float> x((size_t)nc * k), mask((size_t)n * k);
    for (size_t i = 0; i < x.size(); i++) x[i] = i % 5 == 0 ? 0.0f : (float)((int)(i * 7 % 23) - 11) / 8.0f;
    for (size_t i = 0; i < mask.size(); i++) mask[i] = i % 3 == 0 ? 0.0f : 1.0f;

    graphlily::module::SpMMModule mm;
    mm.set_target("hw");
    mm.set_up_runtime("unused.xclbin");
    mm.load_and_format_matrix(a);
    mm.send_matrix_host_to_device();
    mm.send_vectors_host_to_device(x, k);
    mm.send_mask_host_to_device(mask);
    const graphlily::SemiringType semirings[3] = {graphlily::ArithmeticSemiring, graphlily::LogicalSemiring, graphlily::TropicalSemiring};
    const char *names[3] = {"muladd", "andor", "addmin"};
    const graphlily::MaskType masks[3] = {graphlily::kNoMask, graphlily::kMaskWriteToZero, graphlily::kMaskWriteToOne};
    int bad = 0;
    for (int s = 0; s < 3; s++)
        for (int m = 0; m < 3; m++) {
            mm.set_semiring(semirings[s]);
            mm.set_mask_type(masks[m]);
            mm.run();
            const std::vector<float> y = mm.send_results_device_to_host();
            const float zero = semirings[s].zero;
            int wrong = 0;
            for (uint32_t r = 0; r < n; r++)
                for (uint32_t c = 0; c < k; c++) {
                    double sum = zero, abs_sum = 0;
                    float best = zero;
                    bool hit = false;
                    for (uint32_t e = a.adj_indptr[r]; e < a.adj_indptr[r + 1]; e++) {
                        const float xv = x[(size_t)a.adj_indices[e] * k + c];
                        sum += (double)a.adj_data[e] * (double)xv;
                        abs_sum += std::fabs((double)a.adj_data[e] * (double)xv);
                        best = a.adj_data[e] + xv < best ? a.adj_data[e] + xv : best;
                        hit |= xv != 0.0f;
                    }
                    const float mv = mask[(size_t)r * k + c], got = y[(size_t)r * k + c];
                    const bool keep = m == 0 || (m == 1 ? mv == 0.0f : mv != 0.0f);
                    const double len = a.adj_indptr[r + 1] - a.adj_indptr[r];
                    const bool ok = !keep ? got == 0.0f
                                    : s == 0 ? std::fabs(got - sum) <= std::ldexp(std::fabs(sum), -24) + len * std::ldexp(abs_sum, -52) + std::ldexp(1.0, -149)
                                    : s == 1 ? got == (hit ? 1.0f : zero)
                                             : got == best;
                    if (!ok && !wrong++) printf("%s mask %d: Y[%u, %u] is %g\n", names[s], m, r, c, got);
                }
            printf("%s mask %d: short %llu wavefront %llu workgroup %llu tiles %llu, %d wrong\n", names[s], m, (unsigned long long)mm.stats()[0],
                   (unsigned long long)mm.stats()[1], (unsigned long long)mm.stats()[2], (unsigned long long)mm.stats()[3], wrong);
            bad |= wrong != 0;
        }
    if (!bad) printf("SpMM OK\n");
    return bad;
}
