// graphlily/module/spgemm_module.h -- SpGEMMModule on MI355X (an extension: the reference has no such module; the C++ twin of
// SpGEMMModule in graphlily_amd/module.py): C = A (+).(x) B with a sparse result under the three semirings, with an optional
// structural mask, through gl_spgemm_symbolic / gl_spgemm_numeric (include/graphlily_hip_spgemm.h).  The
// interface mirrors SpMVModule's.  A, B and the masks are square matrices over the same vertices.  The plans are boolean plans
// of all-ones values -- a zero VALUE is a legitimate value here, and the row copy would store it as no entry -- and the values
// travel in buffers of their own, in the order of the sorted rows.  Errors print and exit, as in the modules next to it.
#ifndef GRAPHLILY_SPGEMM_MODULE_H_
#define GRAPHLILY_SPGEMM_MODULE_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "graphlily/global.h"
#include "graphlily_hip_spgemm.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/module/base_module.h"

using graphlily::io::CSRMatrix;

namespace graphlily {
namespace module {

class SpGEMMModule : public BaseModule {
    SemiringType semiring_ = ArithmeticSemiring;
    MaskType mask_type_ = kNoMask;
    size_t mask_slot_ = 0;
    CSRMatrix<float> a_, b_;                            // rows strictly ascending
    bool b_is_a_ = true;
    std::vector<CSRMatrix<float>> masks_;               // by slot; a slot that was never loaded has num_rows == 0 and no plan
    gl_spmv_plan plan_a_ = nullptr, plan_b_ = nullptr;
    std::vector<gl_spmv_plan> plan_masks_;
    uint64_t stats_[4] = {0, 0, 0, 0};
    uint32_t nnz_ = 0;

    static void fail_(const char *what) {
        printf("SpGEMMModule: %s\n", what);
        exit(EXIT_FAILURE);
    }
    // -> the square matrix with the columns of every row ascending, the values carried along; a duplicate entry is refused
    static CSRMatrix<float> sorted_rows_(CSRMatrix<float> const &m) {
        if (m.num_rows != m.num_cols) fail_("rectangular operands are out of scope");
        CSRMatrix<float> out = m;
        out.adj_indptr.resize((size_t)m.num_rows + 1);
        const size_t nnz = out.adj_indptr[m.num_rows];
        out.adj_indices.resize(nnz);
        out.adj_data.resize(nnz);
        std::vector<std::pair<uint32_t, float>> row;
        for (uint32_t v = 0; v < m.num_rows; v++) {
            row.clear();
            for (uint32_t i = m.adj_indptr[v]; i < m.adj_indptr[v + 1]; i++) row.push_back(std::make_pair(m.adj_indices[i], m.adj_data[i]));
            std::stable_sort(row.begin(), row.end(), [](std::pair<uint32_t, float> const &x, std::pair<uint32_t, float> const &y) { return x.first < y.first; });
            for (size_t i = 0; i < row.size(); i++) {
                if (i && row[i].first == row[i - 1].first) fail_("an entry is stored twice");
                out.adj_indices[m.adj_indptr[v] + i] = row[i].first;
                out.adj_data[m.adj_indptr[v] + i] = row[i].second;
            }
        }
        return out;
    }
    static gl_spmv_plan ones_plan_(CSRMatrix<float> const &m) {
        gl_spmv_plan p = nullptr;
        const std::vector<float> ones(m.adj_indices.size(), 1.0f);
        GRAPHLILY_CHECK(gl_spmv_plan_create_ex(&p, m.num_rows, m.num_cols, m.adj_indptr.data(), m.adj_indices.data(), ones.data(), 0,
                                               m.num_rows, GL_PLAN_BOOLEAN | GL_PLAN_NO_MULADD));
        return p;
    }
    static DeviceBuffer upload_values_(CSRMatrix<float> const &m) {
        const size_t nnz = m.adj_data.size();
        DeviceBuffer buf(sizeof(float) * (nnz ? nnz : 1));
        if (nnz) buf.upload(m.adj_data.data(), sizeof(float) * nnz);
        return buf;
    }
    void destroy_plans_() {
        if (plan_b_ != plan_a_) gl_spmv_plan_destroy(plan_b_);
        gl_spmv_plan_destroy(plan_a_);
        for (gl_spmv_plan p : plan_masks_) gl_spmv_plan_destroy(p);
        plan_a_ = plan_b_ = nullptr;
        plan_masks_.clear();
    }

public:
    DeviceBuffer a_val_buf, b_val_buf;                  // an f32 per entry of the sorted rows
    DeviceBuffer c_indptr_buf, c_indices_buf, c_val_buf;

    SpGEMMModule() : BaseModule("overlay") {}
    ~SpGEMMModule() override { destroy_plans_(); }

    void set_semiring(SemiringType semiring) { semiring_ = semiring; }
    // kNoMask; kMaskWriteToOne: C is written where the matrix of load_mask_matrix(csr, slot) stores an entry; kMaskWriteToZero:
    // where it stores none (the complement) -- SpMVModule's reading of the two, with "stored" for "non-zero"
    void set_mask_type(MaskType mask_type, size_t slot = 0) {
        mask_type_ = mask_type;
        mask_slot_ = slot;
    }
    uint32_t get_num_rows() const { return a_.num_rows; }
    uint32_t get_nnz() const { return nnz_; }           // of C, after run()
    const uint64_t *stats() const { return stats_; }    // of the symbolic call: nnz(C), products, rows in the workgroup / slab path

    void load_and_format_matrices(CSRMatrix<float> const &a) {
        a_ = sorted_rows_(a);
        b_ = CSRMatrix<float>();
        b_is_a_ = true;
    }
    void load_and_format_matrices(CSRMatrix<float> const &a, CSRMatrix<float> const &b) {
        a_ = sorted_rows_(a);
        b_ = sorted_rows_(b);
        b_is_a_ = false;
        if (b_.num_rows != a_.num_rows) fail_("A and B are over different vertices");
    }
    // several masks may be loaded, one per slot: they share the plans of A and B
    void load_mask_matrix(CSRMatrix<float> const &mask, size_t slot = 0) {
        if (masks_.size() <= slot) masks_.resize(slot + 1);
        masks_[slot] = sorted_rows_(mask);
    }

    void send_matrices_host_to_device() {
        barrier_();
        destroy_plans_();
        plan_a_ = ones_plan_(a_);
        a_val_buf = upload_values_(a_);
        plan_b_ = b_is_a_ ? plan_a_ : ones_plan_(b_);
        b_val_buf = b_is_a_ ? a_val_buf : upload_values_(b_);
        for (CSRMatrix<float> const &m : masks_) {
            if (m.adj_indptr.size() && m.num_rows != a_.num_rows) fail_("a mask is over other vertices than the operands");
            plan_masks_.push_back(m.adj_indptr.size() ? ones_plan_(m) : nullptr);
        }
        finish_();
    }

    // symbolic, then the buffers of C, then numeric.  NaN values are refused under every semiring, +-inf under (+,x).
    void run() {
        if (!plan_a_) fail_("run: send_matrices_host_to_device first");
        if (semiring_.op != kLogicalAndOr)
            for (CSRMatrix<float> const *m : {&a_, b_is_a_ ? &a_ : &b_})
                for (float v : m->adj_data)
                    if (std::isnan(v) || (semiring_.op == kMulAdd && std::isinf(v))) fail_("run: a NaN (or, under (+,x), an infinite) value");
        gl_spmv_plan mask = nullptr;
        if (mask_type_ != kNoMask) {
            if (mask_slot_ >= plan_masks_.size() || !plan_masks_[mask_slot_]) fail_("run: load_mask_matrix before send_matrices_host_to_device");
            mask = plan_masks_[mask_slot_];
        }
        const uint32_t flags = mask_type_ == kMaskWriteToZero ? GL_SPGEMM_MASK_COMPLEMENT : 0u;
        barrier_();
        c_indptr_buf = DeviceBuffer(sizeof(uint32_t) * ((size_t)a_.num_rows + 1));
        GRAPHLILY_CHECK(gl_spgemm_symbolic(plan_a_, plan_b_, mask, flags, (uint32_t *)c_indptr_buf.ptr(), stats_));
        nnz_ = (uint32_t)stats_[0];
        c_indices_buf = DeviceBuffer(sizeof(uint32_t) * (nnz_ ? nnz_ : 1));
        c_val_buf = DeviceBuffer(sizeof(float) * (nnz_ ? nnz_ : 1));
        GRAPHLILY_CHECK(gl_spgemm_numeric(plan_a_, plan_b_, mask, flags, (uint32_t)semiring_.op, (const float *)a_val_buf.rptr(),
                                          (const float *)b_val_buf.rptr(), (const uint32_t *)c_indptr_buf.rptr(),
                                          (uint32_t *)c_indices_buf.ptr(), (float *)c_val_buf.ptr(), nullptr));
        finish_();
    }

    // -> C, the columns of every row ascending; under (||,&&) every value is 1
    CSRMatrix<float> send_results_device_to_host() {
        CSRMatrix<float> c{a_.num_rows, a_.num_rows, std::vector<float>(nnz_), std::vector<uint32_t>(nnz_),
                           std::vector<uint32_t>((size_t)a_.num_rows + 1)};
        c_indptr_buf.download(c.adj_indptr.data(), sizeof(uint32_t) * c.adj_indptr.size());
        if (nnz_) {
            c_indices_buf.download(c.adj_indices.data(), sizeof(uint32_t) * nnz_);
            c_val_buf.download(c.adj_data.data(), sizeof(float) * nnz_);
        }
        return c;
    }
};

}  // namespace module
}  // namespace graphlily

#endif  // GRAPHLILY_SPGEMM_MODULE_H_
