// graphlily/app/pagerank.h -- PageRank over the MI355X backend with the reference's class (graphlily/app/pagerank.h:17-160
// of the reference: same name, constructor, public methods), so that benchmark/bench_pagerank.cpp compiles unmodified with
// -I<this repo>/include in front.  The rank vector starts on the DEVICE (the reference builds n floats on the host and uploads
// them per call, pagerank.h:81-82); an iteration -- SpMV, then eWiseAdd of the teleport term, results -> vector (:84-88) -- runs
// as ONE SpMV whose epilogue adds the teleport term (passed as the semiring's zero: zero + sum is the float eWiseAdd produces)
// and a swap of the two buffers (module/fusion.h, for modules owned by a ModuleCollection).
// -DGRAPHLILY_USE_REFERENCE_APPS: the next graphlily/app/pagerank.h on the include path (the reference checkout's) instead.
#if defined(GRAPHLILY_USE_REFERENCE_APPS)
#include_next "graphlily/app/pagerank.h"
#else
#ifndef GRAPHLILY_HIP_APP_PAGERANK_H_
#define GRAPHLILY_HIP_APP_PAGERANK_H_
#define GRAPHLILY_APP_PAGERANK_H_   // (the reference's guard)

#include "graphlily/app/module_collection.h"
#include "graphlily/module/spmv_module.h"
#include "graphlily/module/add_scalar_vector_dense_module.h"
#include "graphlily/io/data_loader.h"
#include "graphlily/io/data_formatter.h"

#include <chrono>
#include <cmath>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace graphlily {
namespace app {

class PageRank : public app::ModuleCollection {
private:
    graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *SpMV_;
    graphlily::module::eWiseAddModule<graphlily::val_t> *eWiseAdd_;
    uint32_t matrix_num_rows_ = 0, matrix_num_cols_ = 0;
    uint32_t num_channels_, spmv_out_buf_len_, vec_buf_len_;
    graphlily::SemiringType semiring_ = graphlily::ArithmeticSemiring;
    using aligned_dense_vec_t = graphlily::aligned_dense_vec_t;
    using aligned_sparse_vec_t = graphlily::aligned_sparse_vec_t;
    using aligned_dense_float_vec_t = graphlily::aligned_dense_float_vec_t;
    typedef graphlily::value_kind<graphlily::val_t> VK;
    // solve(): what load_and_format_matrix leaves for it, and what the last solve() found
    uint32_t n_real_ = 0;
    float damping_ = 0;
    std::vector<uint32_t> dangling_bits_;
    uint32_t iterations_ = 0;
    bool converged_ = false;
    std::vector<double> residuals_;

    // rank = 1 / n everywhere (over the PADDED n, pagerank.h:81), on the device
    void start_() {
        const graphlily::val_t r0 = 1.0 / matrix_num_rows_;
        DeviceBuffer rank(sizeof(graphlily::val_t) * (size_t)matrix_num_rows_);
        GRAPHLILY_CHECK(gl_buf_fill_u32((uint32_t *)rank.ptr(), VK::bits(r0), matrix_num_rows_));
        SpMV_->bind_vector_buf(rank);
        eWiseAdd_->bind_in_buf(SpMV_->results_buf);
        eWiseAdd_->bind_out_buf(SpMV_->vector_buf);
    }

public:
    PageRank(uint32_t num_channels, uint32_t spmv_out_buf_len, uint32_t vec_buf_len)
        : num_channels_(num_channels), spmv_out_buf_len_(spmv_out_buf_len), vec_buf_len_(vec_buf_len) {
        SpMV_ = new graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t>(num_channels_, spmv_out_buf_len_, vec_buf_len_);
        SpMV_->set_semiring(semiring_);
        SpMV_->set_mask_type(graphlily::kNoMask);
        add_module(SpMV_);
        eWiseAdd_ = new graphlily::module::eWiseAddModule<graphlily::val_t>();
        add_module(eWiseAdd_);
    }

    uint32_t get_nnz() { return SpMV_->get_nnz(); }

    void load_and_format_matrix(std::string csr_float_npz_path, float damping, bool skip_empty_rows) {
        CSRMatrix<float> csr_matrix = graphlily::io::load_csr_matrix_from_float_npz(csr_float_npz_path);
        n_real_ = csr_matrix.num_rows;
        damping_ = damping;
        graphlily::io::util_round_csr_matrix_dim(csr_matrix, num_channels_ * graphlily::pack_size, num_channels_ * graphlily::pack_size);
        graphlily::io::util_normalize_csr_matrix_by_outdegree(csr_matrix);
        for (auto &x : csr_matrix.adj_data) x = x * damping;
        // the dangling set of solve(): the columns of the padded matrix without a stored entry, bit v % 32 of word v / 32
        dangling_bits_.assign(((size_t)csr_matrix.num_cols + 31) / 32, 0xffffffffu);
        for (const auto c : csr_matrix.adj_indices) dangling_bits_[c >> 5] &= ~(1u << (c & 31u));
        SpMV_->load_and_format_matrix(csr_matrix, skip_empty_rows);
        matrix_num_rows_ = SpMV_->get_num_rows();
        matrix_num_cols_ = SpMV_->get_num_cols();
        assert(matrix_num_rows_ == matrix_num_cols_);
    }

    void send_matrix_host_to_device() { SpMV_->send_matrix_host_to_device(); }

    aligned_dense_vec_t pull(graphlily::val_t damping, uint32_t num_iterations) {
        start_();
        SpMV_->chain(true);   // every result is the next vector: the run's epilogue prepares the next run's packed x
        for (uint32_t iter = 1; iter <= num_iterations; iter++) {
            SpMV_->run();
            eWiseAdd_->run(matrix_num_rows_, (1 - damping) / matrix_num_rows_);   // the teleport term, the reference's expression (:87)
        }
        aligned_dense_vec_t rank = SpMV_->send_vector_device_to_host();
        SpMV_->chain(false);
        return rank;
    }

    // Extension: PageRank proper -- personalised teleport, the rank of vertices without out-edges handed back
    // through the teleport term, and a residual stop.  With M the prepared matrix, D the columns of the padded matrix without
    // an entry, p the personalisation (>= 0, length = the matrix's own row count or the padded one and 0 on padding, normalised
    // here in double to sum 1, then cast; empty = 1 / n0 on the n0 real vertices) and d = (float)damping:
    //   x_0 = p;  c_k = (float)((1 - d) + d * sum_{u in D} x_k[u]);  x_{k+1} = fl32(M x_k + fl32(c_k * p));
    //   r_{k+1} = sum_v |x_{k+1}[v] - x_k[v]|     (sums in double)
    // until r <= tol or max_iterations.  An iteration is the (+,x) SpMV and gl_pagerank_update; both sums stay on the device, the
    // control block is read back every `check_every` iterations, and iterations enqueued past convergence leave the vector
    // alone: the result does not depend on check_every.  Misuse throws std::invalid_argument.
    aligned_dense_float_vec_t solve(float damping, double tol, uint32_t max_iterations,
                                    const std::vector<float> &personalization = std::vector<float>(), uint32_t check_every = 4) {
        const uint32_t n = matrix_num_rows_, n0 = n_real_;
        if (VK::kind != GL_VAL_FLOAT) throw std::invalid_argument("PageRank::solve: float values only");
        if (damping != damping_) throw std::invalid_argument("PageRank::solve: damping differs from the one the matrix was prepared with");
        if (!(tol >= 0)) throw std::invalid_argument("PageRank::solve: tol < 0");
        if (max_iterations < 1 || max_iterations > GL_PAGERANK_MAX_SLOTS) throw std::invalid_argument("PageRank::solve: max_iterations out of range");
        if (check_every < 1) throw std::invalid_argument("PageRank::solve: check_every < 1");
        std::vector<float> p(n, 0.0f);
        if (personalization.empty()) {
            for (uint32_t v = 0; v < n0; v++) p[v] = (float)(1.0 / n0);
        } else {
            if (personalization.size() != n0 && personalization.size() != n) throw std::invalid_argument("PageRank::solve: personalization has the wrong length");
            double total = 0;
            for (size_t v = 0; v < personalization.size(); v++) {
                const float g = personalization[v];
                if (!std::isfinite(g) || g < 0) throw std::invalid_argument("PageRank::solve: personalization has a negative or non-finite entry");
                if (v >= n0 && g != 0) throw std::invalid_argument("PageRank::solve: personalization is not 0 on the padding vertices");
                total += (double)g;      // (in index order, like the Python driver's)
            }
            if (!(total > 0) || !std::isfinite(total)) throw std::invalid_argument("PageRank::solve: personalization has zero sum");
            for (uint32_t v = 0; v < n0; v++) p[v] = (float)((double)personalization[v] / total);
        }
        const uint32_t slots = max_iterations;
        size_t ctl_bytes = 0;
        GRAPHLILY_CHECK(gl_pagerank_ctl_bytes(slots, &ctl_bytes));
        const size_t head_bytes = 16 + 16 * ((size_t)slots + 1);
        DeviceBuffer p_buf(sizeof(float) * (size_t)n), bits_buf(sizeof(uint32_t) * dangling_bits_.size()), ctl(ctl_bytes);
        DeviceBuffer x(sizeof(float) * (size_t)n), y(sizeof(float) * (size_t)n);
        p_buf.upload(p.data(), sizeof(float) * (size_t)n);
        bits_buf.upload(dangling_bits_.data(), sizeof(uint32_t) * dangling_bits_.size());
        GRAPHLILY_CHECK(gl_pagerank_begin((const float *)p_buf.rptr(), n, (const uint32_t *)bits_buf.rptr(), (float *)x.ptr(), ctl.ptr(), slots));
        // the module's bindings are put back however this function is left (pull() is what it was); the semiring is the
        // module's own all along: (+,x) with zero = 0, and no chaining -- the update rewrites every result
        struct Rebind {
            graphlily::module::SpMVModule<graphlily::val_t, graphlily::val_t> *spmv;
            DeviceBuffer vector, results;
            ~Rebind() {
                spmv->bind_vector_buf(vector);
                spmv->bind_results_buf(results);
            }
        } rebind = {SpMV_, SpMV_->vector_buf, SpMV_->results_buf};
        (void)rebind;
        SpMV_->set_semiring(semiring_);
        uint32_t k = 0, done = 0;
        while (k < max_iterations && !done) {
            for (uint32_t b = std::min(check_every, max_iterations - k); b; b--) {
                k++;
                SpMV_->bind_vector_buf(x);
                SpMV_->bind_results_buf(y);
                SpMV_->run();
                // (y.ptr(): a run the module layer held back for an eWiseAdd to follow runs now, as it is)
                GRAPHLILY_CHECK(gl_pagerank_update((float *)y.ptr(), (const float *)x.rptr(), (const float *)p_buf.rptr(),
                                                   (const uint32_t *)bits_buf.rptr(), n, damping, tol, ctl.ptr(), k));
                std::swap(x, y);
            }
            GRAPHLILY_CHECK(gl_buf_d2h(&done, ctl.rptr(), sizeof(done)));
        }
        std::vector<double> head(head_bytes / 8);
        GRAPHLILY_CHECK(gl_buf_d2h(head.data(), ctl.rptr(), head_bytes));
        const uint32_t *words = reinterpret_cast<const uint32_t *>(head.data());
        converged_ = words[0] != 0;
        iterations_ = words[1];
        residuals_.assign(head.begin() + 2 + (slots + 1) + 1, head.begin() + 2 + (slots + 1) + 1 + iterations_);
        aligned_dense_float_vec_t rank(n);
        x.download(rank.data(), sizeof(float) * (size_t)n);
        return rank;
    }
    uint32_t iterations() const { return iterations_; }
    bool converged() const { return converged_; }
    const std::vector<double> &residuals() const { return residuals_; }

    // the reference's buckets (pagerank.h:93-147), every call followed by a device synchronisation
    aligned_dense_vec_t pull_time_breakdown(graphlily::val_t damping, uint32_t num_iterations) {
        typedef std::chrono::high_resolution_clock clk;
        float spmv_ms = 0, ewise_ms = 0, transfer_ms = 0;
        auto timed = [](float &bucket, const std::function<void()> &fn) {
            GRAPHLILY_CHECK(gl_sync());
            const auto t0 = clk::now();
            fn();
            GRAPHLILY_CHECK(gl_sync());
            bucket += float(std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count()) / 1000;
        };
        const auto start = clk::now();
        timed(transfer_ms, [&] { start_(); });
        for (uint32_t iter = 1; iter <= num_iterations; iter++) {
            timed(spmv_ms, [&] { SpMV_->run(); GRAPHLILY_CHECK(gl_sync()); });
            timed(ewise_ms, [&] { eWiseAdd_->run(matrix_num_rows_, (1 - damping) / matrix_num_rows_); });
        }
        aligned_dense_vec_t result;
        timed(transfer_ms, [&] { result = SpMV_->send_vector_device_to_host(); });
        const float total_ms = float(std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - start).count()) / 1000;
        std::cout << "total_time_ms per iteration: " << total_ms / num_iterations << std::endl;
        std::cout << "spmv_time_ms per iteration: " << spmv_ms / num_iterations << std::endl;
        std::cout << "ewise_time_ms per iteration: " << ewise_ms / num_iterations << std::endl;
        std::cout << "data_transfer_time_ms per iteration: " << transfer_ms / num_iterations << std::endl;
        return result;
    }

    aligned_dense_float_vec_t compute_reference_results(float damping, uint32_t num_iterations) {
        aligned_dense_float_vec_t rank(matrix_num_rows_, 1.0 / matrix_num_rows_);
        for (uint32_t iter = 1; iter <= num_iterations; iter++) {
            rank = SpMV_->compute_reference_results(rank);
            rank = eWiseAdd_->compute_reference_results(rank, matrix_num_rows_, (1 - damping) / matrix_num_rows_);
        }
        return rank;
    }
};

}  // namespace app
}  // namespace graphlily

#endif  // GRAPHLILY_HIP_APP_PAGERANK_H_
#endif  // GRAPHLILY_USE_REFERENCE_APPS
