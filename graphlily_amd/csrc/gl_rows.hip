// The contract of the row copy (gl_rows.h): the refusals, and the three kernels that establish what the plan caches about its
// rows -- rows_sorted, rows_are_sets, rows_symmetric.  Each check runs once per plan, over four control words of its own, and
// waits for its answer.  Also the one kernel that numbers an array (rows_iota).
#include "gl_rows.h"

namespace gl {

constexpr uint32_t kNoColumn = 0xffffffffu;    // a zero-valued entry

// do the valid (!= 0xffffffff) columns of every row ascend?  a wavefront per row
__global__ __launch_bounds__(256) void rows_sorted_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                          uint32_t rows, uint32_t nz_base, uint32_t *__restrict__ unsorted) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool bad = false;
    for (uint32_t r = blockIdx.x * 4u + wave; r < rows; r += gridDim.x * 4u) {
        const uint32_t beg = row_ptr[r] - nz_base, end = row_ptr[r + 1u] - nz_base;
        for (uint32_t k = beg + 1u + lane; k < end; k += 64u) {
            const uint32_t cur = row_idx[k];
            if (cur == kNoColumn) continue;
            uint32_t j = k - 1u, prev = row_idx[j];
            while (prev == kNoColumn && j > beg) prev = row_idx[--j];
            bad |= prev != kNoColumn && prev > cur;
        }
    }
    if (__any(bad) && lane == 0) atomicOr(unsorted, 1u);
}

// Are the rows strictly ascending sets of columns below num_cols?  The descents of the whole entry list are counted, and so
// are those that sit on a row boundary: the rows ascend iff the two counts agree.  ctl[0]: a column >= num_cols (0xffffffff:
// zero-valued), ctl[1]: descents, ctl[2]: descents on row boundaries
__global__ __launch_bounds__(256) void rows_sets_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                        uint32_t rows, uint32_t nnz, uint32_t nz_base, uint32_t num_cols,
                                                        uint32_t *__restrict__ ctl) {
    uint32_t bad = 0, descents = 0, allowed = 0;
    const uint32_t stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    for (uint64_t k = first; k < nnz; k += stride) {
        const uint32_t c = row_idx[k];
        bad |= c >= num_cols ? 1u : 0u;
        if (k != 0u) descents += row_idx[k - 1u] >= c ? 1u : 0u;
    }
    for (uint64_t r = first; r < rows; r += stride) {
        const uint32_t b = row_ptr[r] - nz_base, e = row_ptr[r + 1u] - nz_base;     // (offsets into the caller's entry list)
        if (b != 0u && b < e) allowed += row_idx[b - 1u] >= row_idx[b] ? 1u : 0u;
    }
    if (bad) atomicOr(ctl, 1u);
    if (descents) atomicAdd(ctl + 1, descents);
    if (allowed) atomicAdd(ctl + 2, allowed);
}

// behind the sets check (every column is < n): is (u, v) stored for every (v, u)?  A wavefront per row.  (u, v) is looked up in
// the PARTNER's rows: the plan's own for the symmetry verdict, another plan's for "is that plan the transpose", which also looks
// the diagonal entries up.
__global__ __launch_bounds__(256) void rows_transpose_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                             uint32_t n, uint32_t nz_base, const uint32_t *__restrict__ prow_ptr,
                                                             const uint32_t *__restrict__ prow_idx, uint32_t pnz_base, bool self,
                                                             uint32_t *__restrict__ verdict) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool bad = false;
    for (uint64_t v = blockIdx.x * 4u + wave; v < n; v += gridDim.x * 4u) {
        const uint32_t b = row_ptr[v] - nz_base, e = row_ptr[v + 1u] - nz_base;
        for (uint64_t j = (uint64_t)b + lane; j < e; j += 64u) {
            const uint32_t u = row_idx[j];
            if (self && u == (uint32_t)v) continue;
            const uint32_t ub = prow_ptr[u] - pnz_base, lu = prow_ptr[u + 1u] - pnz_base - ub;
            bad |= lu == 0u || prow_idx[ub + rows_lower_bound(prow_idx + ub, lu, (uint32_t)v)] != (uint32_t)v;
        }
    }
    if (bad) atomicOr(verdict, 1u);
}

__global__ __launch_bounds__(256) void rows_iota_kernel(uint32_t *__restrict__ out, uint32_t n) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) out[v] = (uint32_t)v;
}

int rows_iota(uint32_t *d_out, uint32_t n) {
    rows_iota_kernel<<<rows_stream_grid(n), 256, 0, ctx().stream>>>(d_out, n);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// launch(ctl, stream) enqueues one check kernel over four zeroed control words; -> their values (one synchronisation)
template <typename Launch>
static int rows_run_check(uint32_t (&h)[4], Launch launch) {
    hipStream_t s = ctx().stream;
    uint32_t *ctl = nullptr;
    GL_HIP(hipMalloc((void **)&ctl, sizeof(h)));
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(h), s);
    if (e == hipSuccess) {
        launch(ctl, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, s);
    const hipError_t w = hipStreamSynchronize(s);     // (waited for whether or not the copy could be enqueued: h is on the stack)
    (void)hipFree(ctl);
    GL_HIP(e != hipSuccess ? e : w);
    return GL_OK;
}

int rows_check_sorted(gl_spmv_plan p) {
    if (p->rows_sorted >= 0) return GL_OK;
    const RowsView r = rows_view(p);
    uint32_t h[4] = {0, 0, 0, 0};
    if (r.rows) {
        const unsigned grid = std::min<unsigned>(cdiv(r.rows, 4u), (unsigned)ctx().num_cus * 32u);
        const int rc = rows_run_check(h, [&](uint32_t *ctl, hipStream_t s) {
            rows_sorted_kernel<<<grid, 256, 0, s>>>(r.row_ptr, r.row_idx, r.rows, r.nz_base, ctl);
        });
        if (rc != GL_OK) return rc;
    }
    p->rows_sorted = h[0] ? 0 : 1;
    return GL_OK;
}

static int rows_check_sets(gl_spmv_plan p) {
    if (p->rows_are_sets >= 0) return GL_OK;
    const RowsView r = rows_view(p);
    const uint32_t nnz = (uint32_t)p->nnz;
    uint32_t h[4] = {0, 0, 0, 0};
    const unsigned grid = std::max(1u, std::min<unsigned>(cdiv(std::max(nnz, r.rows), 256u), (unsigned)ctx().num_cus * 16u));
    const int rc = rows_run_check(h, [&](uint32_t *ctl, hipStream_t s) {
        rows_sets_kernel<<<grid, 256, 0, s>>>(r.row_ptr, r.row_idx, r.rows, nnz, r.nz_base, r.num_cols, ctl);
    });
    if (rc != GL_OK) return rc;
    p->rows_are_sets = (h[0] == 0u && h[1] == h[2]) ? 1 : 0;
    return GL_OK;
}

int rows_check_transpose(gl_spmv_plan p, gl_spmv_plan partner, bool *ok) {
    const RowsView r = rows_view(p), q = rows_view(partner);
    uint32_t h[4] = {0, 0, 0, 0};
    const unsigned grid = std::max(1u, std::min<unsigned>(cdiv(r.rows, 4u), (unsigned)ctx().num_cus * 16u));
    const int rc = rows_run_check(h, [&](uint32_t *ctl, hipStream_t s) {
        rows_transpose_kernel<<<grid, 256, 0, s>>>(r.row_ptr, r.row_idx, r.rows, r.nz_base, q.row_ptr, q.row_idx, q.nz_base, partner == p, ctl);
    });
    *ok = rc == GL_OK && h[0] == 0u;
    return rc;
}

int rows_require(gl_spmv_plan p, unsigned need, const char *who, const char *which, const char *hint) {
    // (a matrix without entries is planned in the general layout whatever the flags, and keeps no row copy: to the callers
    // that ask for a square matrix it is the empty graph)
    if ((p->nnz != 0 || !(need & kRowsSquare)) && (!p->d_csr_indptr || !p->d_csr_indices))
        return set_error(GL_ERR_UNSUPPORTED, "%s: %s keeps no row copy (a GL_PLAN_BOOLEAN plan in the (||,&&) layout does)", who, which);
    if ((need & kRowsIndexable) && p->row_end > p->num_cols)
        return set_error(GL_ERR_UNSUPPORTED, "%s: %s: a vector of num_cols words is indexed by row and by column: needs num_rows <= num_cols",
                         who, which);
    if (!(need & kRowsSquare)) return GL_OK;
    if (p->num_rows != p->num_cols)
        return set_error(GL_ERR_UNSUPPORTED, "%s: %s: rows and columns name the same vertices: needs num_rows == num_cols (%u x %u)", who,
                         which, p->num_rows, p->num_cols);
    if (p->row_begin != 0u || p->row_end != p->num_rows)
        return set_error(GL_ERR_UNSUPPORTED, "%s: %s is a row shard [%u, %u) of %u rows: row u must be readable for every column u", who,
                         which, p->row_begin, p->row_end, p->num_rows);
    if (p->nnz > 0xffffffffull)
        return set_error(GL_ERR_UNSUPPORTED, "%s: %s: %llu entries do not fit 32-bit offsets", who, which, (unsigned long long)p->nnz);
    if (p->nnz == 0) return GL_OK;
    int rc = GL_OK;
    if ((need & kRowsSets) == kRowsSets) {
        if ((rc = rows_check_sets(p)) != GL_OK) return rc;
        if (p->rows_are_sets == 0)
            return set_error(GL_ERR_UNSUPPORTED, "%s: the rows of %s must be strictly ascending sets of columns below num_cols (no duplicate, "
                             "no zero-valued entry, which the row copy stores as column 0xffffffff): %s prepares such a matrix", who, which, hint);
    }
    if ((need & kRowsSymmetric) == kRowsSymmetric) {
        if (p->rows_symmetric < 0) {
            bool ok = false;
            if ((rc = rows_check_transpose(p, p, &ok)) != GL_OK) return rc;
            p->rows_symmetric = ok ? 1 : 0;
        }
        if (p->rows_symmetric == 0)
            return set_error(GL_ERR_UNSUPPORTED, "%s: the pattern of %s is not symmetric (an entry (v, u) without (u, v)), and the call reads "
                             "its rows in both directions: %s prepares what it needs", who, which, hint);
    }
    return GL_OK;
}

int rows_require_pair(gl_spmv_plan pin, gl_spmv_plan pout, const char *who, const char *hint) {
    int rc = rows_require(pin, pout == pin ? kRowsSymmetric : kRowsSets, who, "plan_in", hint);
    if (rc == GL_OK && pout != pin) rc = rows_require(pout, kRowsSets, who, "plan_out", hint);
    if (rc != GL_OK) return rc;
    if (pout->num_rows != pin->num_rows)
        return set_error(GL_ERR_UNSUPPORTED, "%s: plan_out is not the transpose of plan_in: %u and %u vertices", who, pout->num_rows, pin->num_rows);
    if (pout == pin) return GL_OK;
    if (pin->bc_partner != pout || pin->bc_partner_uid != pout->uid) {
        // every entry (v, u) of plan_in is an entry (u, v) of plan_out, and there are as many: the rows are sets, so that is a bijection
        bool ok = pin->nnz == pout->nnz;
        if (ok && pin->nnz != 0 && (rc = rows_check_transpose(pin, pout, &ok)) != GL_OK) return rc;
        pin->bc_partner = pout;
        pin->bc_partner_uid = pout->uid;
        pin->bc_transpose_ok = ok ? 1 : 0;
    }
    if (pin->bc_transpose_ok == 0)
        return set_error(GL_ERR_UNSUPPORTED, "%s: plan_out is not the transpose of plan_in (%llu and %llu entries; an entry (v, u) of plan_in "
                         "needs (u, v) in plan_out): %s prepares both", who, (unsigned long long)pout->nnz, (unsigned long long)pin->nnz, hint);
    return GL_OK;
}

}  // namespace gl

int gl_spmv_plan_rows_sorted(gl_spmv_plan plan, int *sorted) {
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && sorted != nullptr);
    int rc = gl::rows_require(plan, gl::kRowsIndexable, "gl_spmv_plan_rows_sorted", "the plan");
    if (rc == GL_OK) rc = gl::rows_check_sorted(plan);
    if (rc != GL_OK) return rc;
    *sorted = plan->rows_sorted;
    return GL_OK;
}
