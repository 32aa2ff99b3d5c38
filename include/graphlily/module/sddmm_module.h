// graphlily/module/sddmm_module.h -- SDDMMModule on MI355X (an extension: the reference has no such module; the C++ twin of
// SDDMMModule in graphlily_amd/module.py): C = A (x) (X (+).(x) Y^T) sampled at A's entries -- one score per stored entry of A
// from the k features of its row (X, num_rows x k) and of its column (Y, num_cols x k) under the three semirings, through
// gl_sddmm (include/graphlily_hip_sddmm.h).  The interface mirrors SpMMModule's.  A may be rectangular and a row
// shard.  results_buf is the plain per-entry buffer, an f32 per entry of the shard's rows in the matrix' order: what SpMMModule
// takes as its a_val_buf.  Errors print and exit, as in the modules next to it.
#ifndef GRAPHLILY_SDDMM_MODULE_H_
#define GRAPHLILY_SDDMM_MODULE_H_

#include <cmath>
#include <cstdint>
#include <vector>

#include "graphlily/global.h"
#include "graphlily_hip_sddmm.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/module/base_module.h"

using graphlily::io::CSRMatrix;

namespace graphlily {
namespace module {

class SDDMMModule : public BaseModule {
    SemiringType semiring_ = ArithmeticSemiring;
    bool scaled_ = true;
    CSRMatrix<float> csr_;
    uint32_t row_begin_ = 0, row_end_ = 0;
    bool sharded_ = false;
    gl_spmv_plan plan_ = nullptr;
    uint32_t k_ = 0;
    uint64_t ldx_ = 0, ldy_ = 0;                        // 0: k
    size_t first_ = 0, count_ = 0;                      // the shard's entries in the matrix' entry list
    bool values_nan_ = false, values_inf_ = false;      // of A's values
    bool features_nan_ = false, features_inf_ = false;  // of an X and Y this module uploaded
    uint64_t stats_[3] = {0, 0, 0};

    static void fail_(const char *what) {
        printf("SDDMMModule: %s\n", what);
        exit(EXIT_FAILURE);
    }
    static void note_(const float *v, size_t n, bool &nan, bool &inf) {
        for (size_t i = 0; i < n; i++) {
            nan |= std::isnan(v[i]);
            inf |= std::isinf(v[i]);
        }
    }
    static DeviceBuffer upload_(const float *v, size_t n) {
        DeviceBuffer buf(sizeof(float) * (n ? n : 1));
        if (n) buf.upload(v, sizeof(float) * n);
        return buf;
    }
    uint32_t r0_() const { return sharded_ ? row_begin_ : 0u; }
    uint32_t r1_() const { return sharded_ ? row_end_ : csr_.num_rows; }

public:
    DeviceBuffer a_val_buf;                             // an f32 per entry of the plan's rows
    DeviceBuffer x_buf, y_buf, results_buf;

    SDDMMModule() : BaseModule("overlay") {}
    ~SDDMMModule() override { gl_spmv_plan_destroy(plan_); }

    void set_semiring(SemiringType semiring) { semiring_ = semiring; }
    // true (the default): the scores are scaled by A's values; false: A gives the pattern only
    void set_scaled(bool scaled) { scaled_ = scaled; }
    // this device owns rows [row_begin, row_end) of the matrix: only those rows' entries are scored
    void set_row_shard(uint32_t row_begin, uint32_t row_end) {
        row_begin_ = row_begin;
        row_end_ = row_end;
        sharded_ = true;
    }
    uint32_t get_num_rows() const { return csr_.num_rows; }
    uint32_t get_num_cols() const { return csr_.num_cols; }
    uint32_t get_num_features() const { return k_; }
    // {rows on the short path, pieces on the piece path, feature tiles} of the last run()
    const uint64_t *stats() const { return stats_; }

    void load_and_format_matrix(CSRMatrix<float> const &csr) { csr_ = csr; }

    // allocates the results buffer, an f32 per entry of the shard's rows, zero-filled
    void send_matrix_host_to_device() {
        barrier_();
        gl_spmv_plan_destroy(plan_);
        plan_ = nullptr;
        const std::vector<float> ones(csr_.adj_indices.size(), 1.0f);
        GRAPHLILY_CHECK(gl_spmv_plan_create_ex(&plan_, csr_.num_rows, csr_.num_cols, csr_.adj_indptr.data(), csr_.adj_indices.data(), ones.data(),
                                               r0_(), r1_(), GL_PLAN_BOOLEAN | GL_PLAN_NO_MULADD));
        first_ = csr_.adj_indptr[r0_()];
        count_ = csr_.adj_indptr[r1_()] - first_;
        values_nan_ = values_inf_ = false;
        note_(csr_.adj_data.data() + first_, count_, values_nan_, values_inf_);
        a_val_buf = upload_(csr_.adj_data.data() + first_, count_);
        results_buf = upload_(std::vector<float>(count_, 0.0f).data(), count_);
        finish_();
    }

    // X: num_rows x k floats, Y: num_cols x k floats, both row-major
    void send_features_host_to_device(std::vector<float> const &x, std::vector<float> const &y, uint32_t k) {
        if (k == 0 || x.size() != (size_t)csr_.num_rows * k || y.size() != (size_t)csr_.num_cols * k)
            fail_("send_features_host_to_device: X must hold num_rows x k and Y num_cols x k values, k >= 1");
        barrier_();
        k_ = k;
        ldx_ = ldy_ = 0;
        features_nan_ = features_inf_ = false;
        note_(x.data(), x.size(), features_nan_, features_inf_);
        note_(y.data(), y.size(), features_nan_, features_inf_);
        x_buf = upload_(x.data(), x.size());
        y_buf = upload_(y.data(), y.size());
        finish_();
    }
    // device blocks with the leading dimensions ldx, ldy (0: k); what bound blocks hold is the caller's business
    void bind_features_bufs(DeviceBuffer x, DeviceBuffer y, uint32_t k, uint64_t ldx = 0, uint64_t ldy = 0) {
        x_buf = x;
        y_buf = y;
        k_ = k;
        ldx_ = ldx;
        ldy_ = ldy;
        features_nan_ = features_inf_ = false;
    }
    // a device buffer of an f32 per entry of the shard's rows
    void bind_results_buf(DeviceBuffer src) { results_buf = src; }

    // NaN values are refused under every semiring, +-inf under (+,x): of A when its values scale, and of an X and Y this module uploaded
    void run() {
        if (!plan_ || !x_buf.valid() || !y_buf.valid()) fail_("run: send_matrix_host_to_device and send_features_host_to_device first");
        const bool scaled = scaled_ && semiring_.op != kLogicalAndOr;
        const bool nan = features_nan_ || (scaled && values_nan_), inf = features_inf_ || (scaled && values_inf_);
        if (semiring_.op != kLogicalAndOr && (nan || (semiring_.op == kMulAdd && inf))) fail_("run: a NaN (or, under (+,x), an infinite) value");
        barrier_();
        GRAPHLILY_CHECK(gl_sddmm(plan_, scaled ? (const float *)a_val_buf.rptr() : nullptr, (const float *)x_buf.rptr(), ldx_ ? ldx_ : k_,
                                 (const float *)y_buf.rptr(), ldy_ ? ldy_ : k_, (float *)results_buf.ptr(), k_, (int)semiring_.op,
                                 (float)semiring_.zero, stats_));
        finish_();
    }

    // -> A's pattern with the scores as values: the shard's rows filled, the others empty
    CSRMatrix<float> send_results_device_to_host() {
        CSRMatrix<float> c;
        c.num_rows = csr_.num_rows;
        c.num_cols = csr_.num_cols;
        c.adj_data.resize(count_);
        if (count_) results_buf.download(c.adj_data.data(), sizeof(float) * count_);
        c.adj_indices.assign(csr_.adj_indices.begin() + first_, csr_.adj_indices.begin() + first_ + count_);
        for (uint32_t r = 0; r <= csr_.num_rows; r++) {
            const size_t at = csr_.adj_indptr[r] < first_ ? first_ : csr_.adj_indptr[r] > first_ + count_ ? first_ + count_ : csr_.adj_indptr[r];
            c.adj_indptr.push_back((uint32_t)(at - first_));
        }
        return c;
    }

    // the plain host statement of the header: one score per entry of the shard's rows, in the matrix' order; (+,x) in f64
    std::vector<float> compute_reference_results(std::vector<float> const &x, std::vector<float> const &y, uint32_t k) const {
        std::vector<float> out(count_);
        const bool scaled = scaled_ && semiring_.op != kLogicalAndOr;
        const float zero = (float)semiring_.zero;
        for (uint32_t r = r0_(); r < r1_(); r++)
            for (size_t e = csr_.adj_indptr[r]; e < csr_.adj_indptr[r + 1]; e++) {
                const uint32_t j = csr_.adj_indices[e];
                if (j >= csr_.num_cols) {
                    out[e - first_] = 0.0f;
                    continue;
                }
                double sum = zero;
                float best = zero;
                bool hit = false;
                for (uint32_t c = 0; c < k; c++) {
                    const float xv = x[(size_t)r * k + c], yv = y[(size_t)j * k + c];
                    sum += (double)xv * (double)yv;
                    best = xv + yv < best ? xv + yv : best;
                    hit |= xv != 0.0f && yv != 0.0f;
                }
                const float a = csr_.adj_data[e];
                out[e - first_] = semiring_.op == kMulAdd ? (float)(scaled ? (double)a * sum : sum)
                                  : semiring_.op == kAddMin ? (scaled ? a + best : best)
                                                            : (hit ? 1.0f : zero);
            }
        return out;
    }
};

}  // namespace module
}  // namespace graphlily

#endif  // GRAPHLILY_SDDMM_MODULE_H_
