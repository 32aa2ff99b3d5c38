// graphlily::module::SpGEMMModule and graphlily::app::TwoHop driven from C++: every C is printed (its size, then its first row with
// entries) and written as raw words for tests/test_gpu_spgemm.py to compare with the Python layer's, and what needs no second
// opinion is checked here: the offsets start at 0 and never descend, the columns of every row ascend strictly.
//   spgemm_driver graph.npz out_dir          (a square matrix without duplicate entries)
//   g++ -std=c++11 -I<repo>/include tests/cpp/spgemm_driver.cpp -L<repo>/graphlily_amd/lib -lgraphlily_hip
#include "graphlily/app/two_hop.h"

#include <cstdio>
#include <string>
#include <vector>

template <typename T>
static bool write_words(const std::string &path, const std::vector<T> &words) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(words.data(), sizeof(T), words.size(), f) != words.size()) { printf("cannot write %s\n", path.c_str()); return false; }
    fclose(f);
    return true;
}

// -> 0 if C is well formed and was written as out_dir/cpp_<name>_{indptr,indices,val}.bin
static int report(const std::string &out, const std::string &name, const CSRMatrix<float> &c) {
    int bad = c.adj_indptr.size() != (size_t)c.num_rows + 1 || c.adj_indptr[0] != 0 || c.adj_indptr[c.num_rows] != c.adj_indices.size();
    for (uint32_t v = 0; !bad && v < c.num_rows; v++) {
        bad |= c.adj_indptr[v + 1] < c.adj_indptr[v];
        for (uint32_t i = c.adj_indptr[v] + 1; !bad && i < c.adj_indptr[v + 1]; i++) bad |= c.adj_indices[i] <= c.adj_indices[i - 1];
    }
    printf("%s: nnz %zu", name.c_str(), c.adj_indices.size());
    for (uint32_t v = 0; !bad && v < c.num_rows; v++) {
        if (c.adj_indptr[v + 1] == c.adj_indptr[v]) continue;
        printf(", row %u:", v);
        for (uint32_t i = c.adj_indptr[v]; i < c.adj_indptr[v + 1] && i < c.adj_indptr[v] + 8; i++) printf(" (%u, %g)", c.adj_indices[i], c.adj_data[i]);
        break;
    }
    printf(bad ? " MALFORMED\n" : "\n");
    if (!write_words(out + "/cpp_" + name + "_indptr.bin", c.adj_indptr) || !write_words(out + "/cpp_" + name + "_indices.bin", c.adj_indices) ||
        !write_words(out + "/cpp_" + name + "_val.bin", c.adj_data))
        return 2;
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: %s graph.npz out_dir\n", argv[0]); return 2; }
    const std::string npz = argv[1], out = argv[2];
    int bad = 0;
    {
        const CSRMatrix<float> a = graphlily::io::load_csr_matrix_from_float_npz(npz);
        graphlily::module::SpGEMMModule mm;
        mm.set_target("hw");
        mm.set_up_runtime("unused.xclbin");
        mm.load_and_format_matrices(a);
        mm.load_mask_matrix(a);
        mm.send_matrices_host_to_device();
        const graphlily::SemiringType semirings[3] = {graphlily::ArithmeticSemiring, graphlily::LogicalSemiring, graphlily::TropicalSemiring};
        const char *names[3] = {"muladd", "andor", "addmin"};
        const graphlily::MaskType masks[3] = {graphlily::kNoMask, graphlily::kMaskWriteToOne, graphlily::kMaskWriteToZero};
        const char *mask_names[3] = {"none", "mask", "complement"};
        for (int s = 0; s < 3; s++)
            for (int m = 0; m < 3; m++) {
                mm.set_semiring(semirings[s]);
                mm.set_mask_type(masks[m]);
                mm.run();
                bad |= report(out, std::string(names[s]) + "_" + mask_names[m], mm.send_results_device_to_host());
            }
    }
    graphlily::app::TwoHop th;
    th.set_target("hw");
    th.set_up_runtime("unused.xclbin");
    th.load_and_format_matrix(npz);
    th.send_matrix_host_to_device();
    bad |= report(out, "paths", th.run_paths());
    bad |= report(out, "candidates", th.run_candidates());
    if (!bad) printf("SpGEMM OK\n");
    return bad;
}
