// graphlily/module/spmm_module.h -- SpMMModule on MI355X (an extension: the reference has no such module; the C++ twin of
// SpMMModule in graphlily_amd/module.py): Y = A (+).(x) X for a dense block X of k vectors under the three semirings, with an
// optional dense mask of Y's shape, through gl_spmm (include/graphlily_hip_spmm.h) -- one pass over A where k
// SpMVModule runs make k.  The interface mirrors SpMVModule's; X is num_cols x k floats, Y and the mask num_rows x k, all
// row-major.  A may be rectangular and a row shard.  The plan is a boolean plan of all-ones values -- a zero VALUE is a value
// here, and the row copy would store it as no entry -- and the values travel in a buffer of their own, in the matrix' order.
// Errors print and exit, as in the modules next to it.
#ifndef GRAPHLILY_SPMM_MODULE_H_
#define GRAPHLILY_SPMM_MODULE_H_

#include <cmath>
#include <cstdint>
#include <vector>

#include "graphlily/global.h"
#include "graphlily_hip_spmm.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/module/base_module.h"

using graphlily::io::CSRMatrix;

namespace graphlily {
namespace module {

class SpMMModule : public BaseModule {
    SemiringType semiring_ = ArithmeticSemiring;
    MaskType mask_type_ = kNoMask;
    CSRMatrix<float> csr_;
    uint32_t row_begin_ = 0, row_end_ = 0;
    bool sharded_ = false;
    gl_spmv_plan plan_ = nullptr;
    uint32_t k_ = 0;
    uint64_t ldx_ = 0, ldy_ = 0, ldm_ = 0;              // 0: k
    bool values_nan_ = false, values_inf_ = false;      // of A's values and of an X this module uploaded
    uint64_t stats_[4] = {0, 0, 0, 0};

    static void fail_(const char *what) {
        printf("SpMMModule: %s\n", what);
        exit(EXIT_FAILURE);
    }
    void note_(const float *v, size_t n) {
        for (size_t i = 0; i < n; i++) {
            values_nan_ |= std::isnan(v[i]);
            values_inf_ |= std::isinf(v[i]);
        }
    }
    static DeviceBuffer upload_(const float *v, size_t n) {
        DeviceBuffer buf(sizeof(float) * (n ? n : 1));
        if (n) buf.upload(v, sizeof(float) * n);
        return buf;
    }

public:
    DeviceBuffer a_val_buf;                             // an f32 per entry of the plan's rows
    DeviceBuffer vectors_buf, mask_buf, results_buf;

    SpMMModule() : BaseModule("overlay") {}
    ~SpMMModule() override { gl_spmv_plan_destroy(plan_); }

    void set_semiring(SemiringType semiring) { semiring_ = semiring; }
    void set_mask_type(MaskType mask_type) { mask_type_ = mask_type; }
    // this device owns rows [row_begin, row_end) of the matrix: only those rows of Y are written
    void set_row_shard(uint32_t row_begin, uint32_t row_end) {
        row_begin_ = row_begin;
        row_end_ = row_end;
        sharded_ = true;
    }
    uint32_t get_num_rows() const { return csr_.num_rows; }
    uint32_t get_num_cols() const { return csr_.num_cols; }
    uint32_t get_num_vectors() const { return k_; }
    // {rows on the short path, rows on the wavefront path, rows on the workgroup path, column tiles} of the last run()
    const uint64_t *stats() const { return stats_; }

    void load_and_format_matrix(CSRMatrix<float> const &csr) { csr_ = csr; }

    void send_matrix_host_to_device() {
        barrier_();
        gl_spmv_plan_destroy(plan_);
        plan_ = nullptr;
        const uint32_t r0 = sharded_ ? row_begin_ : 0u, r1 = sharded_ ? row_end_ : csr_.num_rows;
        const std::vector<float> ones(csr_.adj_indices.size(), 1.0f);
        GRAPHLILY_CHECK(gl_spmv_plan_create_ex(&plan_, csr_.num_rows, csr_.num_cols, csr_.adj_indptr.data(), csr_.adj_indices.data(), ones.data(),
                                               r0, r1, GL_PLAN_BOOLEAN | GL_PLAN_NO_MULADD));
        const size_t first = csr_.adj_indptr[r0], count = csr_.adj_indptr[r1] - first;
        values_nan_ = values_inf_ = false;
        note_(csr_.adj_data.data() + first, count);
        a_val_buf = upload_(csr_.adj_data.data() + first, count);
        finish_();
    }

    // X: num_cols x k floats, row-major.  Allocates the results buffer for that k, zero-filled, unless one of that size is there.
    void send_vectors_host_to_device(std::vector<float> const &vectors, uint32_t k) {
        if (k == 0 || vectors.size() != (size_t)csr_.num_cols * k) fail_("send_vectors_host_to_device: X must hold num_cols x k values, k >= 1");
        barrier_();
        k_ = k;
        ldx_ = 0;
        note_(vectors.data(), vectors.size());
        vectors_buf = upload_(vectors.data(), vectors.size());
        const size_t out = (size_t)csr_.num_rows * k;
        if (ldy_ != 0 || results_buf.size() != sizeof(float) * (out ? out : 1)) {
            ldy_ = 0;
            results_buf = upload_(std::vector<float>(out, 0.0f).data(), out);
        }
        finish_();
    }
    void send_mask_host_to_device(std::vector<float> const &mask) {
        if (mask.size() != (size_t)csr_.num_rows * k_) fail_("send_mask_host_to_device: the mask must hold num_rows x k values");
        barrier_();
        ldm_ = 0;
        mask_buf = upload_(mask.data(), mask.size());
        finish_();
    }
    // device blocks with a leading dimension `ld` (0: k); what a bound X holds is the caller's business
    void bind_vectors_buf(DeviceBuffer src, uint32_t k, uint64_t ld = 0) {
        vectors_buf = src;
        k_ = k;
        ldx_ = ld;
    }
    void bind_mask_buf(DeviceBuffer src, uint64_t ld = 0) {
        mask_buf = src;
        ldm_ = ld;
    }
    void bind_results_buf(DeviceBuffer src, uint64_t ld = 0) {
        results_buf = src;
        ldy_ = ld;
    }

    // NaN values are refused under every semiring, +-inf under (+,x): of A, and of an X this module uploaded
    void run() {
        if (!plan_ || !vectors_buf.valid()) fail_("run: send_matrix_host_to_device and send_vectors_host_to_device first");
        if (semiring_.op != kLogicalAndOr && (values_nan_ || (semiring_.op == kMulAdd && values_inf_)))
            fail_("run: a NaN (or, under (+,x), an infinite) value");
        if (mask_type_ != kNoMask && !mask_buf.valid()) fail_("run: a mask type without a mask");
        barrier_();
        GRAPHLILY_CHECK(gl_spmm(plan_, semiring_.op == kLogicalAndOr ? nullptr : (const float *)a_val_buf.rptr(), (const float *)vectors_buf.rptr(),
                                ldx_ ? ldx_ : k_, mask_type_ != kNoMask ? (const float *)mask_buf.rptr() : nullptr, ldm_ ? ldm_ : k_,
                                (float *)results_buf.ptr(), ldy_ ? ldy_ : k_, k_, (int)semiring_.op, (float)semiring_.zero, (int)mask_type_, stats_));
        finish_();
    }

    // -> Y, num_rows x k floats, row-major (of a bound buffer with a leading dimension: its k columns)
    std::vector<float> send_results_device_to_host() {
        const size_t n = csr_.num_rows, ld = ldy_ ? ldy_ : k_;
        std::vector<float> flat(n ? (n - 1) * ld + k_ : 0), out(n * k_);
        if (!flat.empty()) results_buf.download(flat.data(), sizeof(float) * flat.size());
        for (size_t r = 0; r < n; r++)
            for (size_t c = 0; c < k_; c++) out[r * k_ + c] = flat[r * ld + c];
        return out;
    }
};

}  // namespace module
}  // namespace graphlily

#endif  // GRAPHLILY_SPMM_MODULE_H_
