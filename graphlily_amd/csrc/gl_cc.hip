// Weakly connected components (gl_cc_begin / gl_cc_hook / gl_cc_finish / gl_cc_labels): lock-free union-find over the plain
// CSR copy that every GL_PLAN_BOOLEAN plan keeps for the bottom-up BFS step (gl_spmv_plan.h: d_csr_indptr / d_csr_indices /
// csr_nz_base), over n = num_cols vertices.
//
//   an entry (v, u) of row v is an edge unless u == 0xffffffff (zero-valued) or u >= n; direction is ignored
//   labels[v] = min { x : x is joined to v by a chain of such edges, taken in either direction }
//   count     = number of v with labels[v] == v
//
// The minimum makes the answer unique: it depends neither on the order of a row's entries nor on the order in which rows,
// shards or plans are hooked, nor on timing.  Begin, hook and finish are separate so that several plans -- the row shards of
// one matrix, two matrices over the same vertices -- can be hooked into ONE parent array before it is finished.
//
// THE INVARIANT: parent[x] <= x at all times, and parent[x] lies in x's component.  Chains strictly descend, so they cannot
// cycle; once every edge is united each component has exactly one root (parent[r] == r), its minimum.
//
// Hook: the walk of gl_rows.h over every row, the wavefront taking over a row longer than `cut` entries;
// shards index through row_begin and csr_nz_base.  For an edge (v, u): find both roots; if they differ,
// atomicCAS(&parent[hi], hi, lo) with hi = max, lo = min.
// MEMORY RULE: gl_rounds.h.  Inside the hook launch:
//   * parent[] is atomic-only: a relaxed atomic load, an atomic min or a compare-and-swap; there is no plain load or store of
//     that array;
//   * a failed compare-and-swap continues from the value it RETURNED (never a re-read): that value is below hi, so every
//     retry strictly descends and progress rests on atomic return values alone -- a stale load can at worst name a vertex
//     that is no longer a root, which the compare-and-swap then refuses;
//   * path shortening is atomicMin(&parent[x], grandparent) only, which keeps the invariant;
//   * the only loops are the descending find and the retry.
// Finish runs behind a launch boundary (plain loads): pointer doubling (gl_unionfind.h, which holds it and the find / unite
// above for gl_bicc.hip too), ping-pong between parent and labels with one device
// "changed" word per round.  A round at least halves the depth, so ceil(log2 n) + 1 rounds suffice; that many are enqueued
// and a round returns at once when its predecessor changed nothing (both arrays then hold the result).  A thread-per-vertex
// walk to the root would not do: a path hooked in index order leaves a chain of length n.  One more pass counts the roots,
// one ballot and one atomic add per wavefront.  No call synchronises with the host.
// NO ROW SKIPPING: entries are stored one way only (row v lists the vertices v is pulled from), so a row skipped because its
// vertex already sits in the giant component (Afforest's shortcut) may hold the only copy of an edge that leaves it.
#include "gl_unionfind.h"

namespace gl {

struct CcHookArgs {
    const uint32_t *row_ptr, *row_idx;
    uint32_t *parent;
    uint32_t row_begin, rows, n, nz_base, cut_steps;
};

__global__ __launch_bounds__(256) void cc_hook_kernel(CcHookArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwords = (a.rows + 63u) >> 6;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += gridDim.x * 4u) {
        const uint32_t local = wd * 64u + lane;
        const bool in = local < a.rows;
        const uint32_t row = a.row_begin + local;     // < n: the plan has row_end <= num_cols
        uint32_t beg = 0, end = 0;
        if (in) {
            beg = a.row_ptr[local] - a.nz_base;
            end = a.row_ptr[local + 1u] - a.nz_base;
        }
        uint32_t anc = row;                           // an ancestor-or-self of `row`: only ever descends
        rows_walk_thread(a.row_idx, beg, end, a.cut_steps, [&](const uint32_t(&c)[4], uint32_t) {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c[u] < a.n && c[u] != row) anc = cc_unite(a.parent, anc, c[u]);
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t v = __shfl(row, src);
            uint32_t av = __shfl(anc, src);                       // (every lane unites from the row's ancestor on its own)
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n && c[u] != v) av = cc_unite(a.parent, av, c[u]);
                return false;
            });
        });
    }
}

__global__ __launch_bounds__(256) void cc_begin_kernel(uint32_t *__restrict__ parent, uint32_t n) {
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) parent[v] = v;
}

__global__ __launch_bounds__(256) void cc_count_kernel(const uint32_t *__restrict__ labels, uint32_t n, uint32_t *__restrict__ count) {
    uint32_t roots = 0;   // per wavefront
    const uint32_t nround = (n + 255u) & ~255u;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += gridDim.x * 256u)
        roots += (uint32_t)__popcll(__ballot(v < n && labels[v] == v));
    if ((threadIdx.x & 63u) == 0u && roots != 0u) atomicAdd(count, roots);
}

int cc_begin(uint32_t *d_parent, uint32_t n) {
    if (!n) return GL_OK;
    cc_begin_kernel<<<rows_stream_grid(n), 256, 0, ctx().stream>>>(d_parent, n);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

int cc_hook(gl_spmv_plan p, uint32_t *d_parent) {
    const uint32_t rows = p->row_end - p->row_begin;
    if (!rows) return GL_OK;
    // A/B knobs (GRAPHLILY_DEBUG, read per call): cc_cut = entries a thread reads before the wavefront takes the row over,
    // cc_grid = workgroups per compute unit
    const RowsWalkShape shape = rows_walk_shape(rows, debug_knob("cc_cut", 32), 1l << 30, debug_knob("cc_grid", 64));
    CcHookArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.parent = d_parent;
    a.row_begin = p->row_begin;
    a.rows = rows;
    a.n = p->num_cols;
    a.nz_base = p->csr_nz_base;
    a.cut_steps = shape.cut_steps;
    cc_hook_kernel<<<shape.grid, 256, 0, ctx().stream>>>(a);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

static int cc_finish(uint32_t *d_parent, uint32_t n, uint32_t *d_labels, uint32_t *d_count, const char *who) {
    hipStream_t s = ctx().stream;
    if (d_count) GL_HIP(hipMemsetAsync(d_count, 0, 4, s));
    if (!n) return GL_OK;
    const int rc = cc_double(d_parent, n, d_labels, who);
    if (rc != GL_OK) return rc;
    const unsigned grid = rows_stream_grid(n);
    if (d_count) {
        cc_count_kernel<<<grid, 256, 0, s>>>(d_labels, n, d_count);
        GL_LAUNCH_CHECK();
    }
    return GL_OK;
}

}  // namespace gl

int gl_cc_begin(uint32_t *d_parent, uint32_t n) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(d_parent != nullptr);
    return gl::cc_begin(d_parent, n);
}

int gl_cc_hook(gl_spmv_plan plan, uint32_t *d_parent) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_parent != nullptr);
    int rc = gl::rows_require(plan, gl::kRowsIndexable, "gl_cc_hook", "the plan");
    if (rc != GL_OK) return rc;
    return gl::cc_hook(plan, d_parent);
}

int gl_cc_finish(uint32_t *d_parent, uint32_t n, uint32_t *d_labels, uint32_t *d_count) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(d_parent != nullptr && d_labels != nullptr);
    GL_ARG(d_labels != d_parent);
    return gl::cc_finish(d_parent, n, d_labels, d_count, "gl_cc_finish");
}

int gl_cc_labels(gl_spmv_plan plan, uint32_t *d_labels, uint32_t *d_count) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_labels != nullptr);
    int rc = gl::rows_require(plan, gl::kRowsIndexable, "gl_cc_labels", "the plan");
    if (rc != GL_OK) return rc;
    const uint32_t n = plan->num_cols;
    if ((rc = gl::plan_scratch(plan->d_cc_scratch, 4u * (size_t)std::max(n, 4u), "gl_cc_labels", "parent scratch")) != GL_OK) return rc;
    if ((rc = gl::cc_begin(plan->d_cc_scratch, n)) != GL_OK) return rc;
    if ((rc = gl::cc_hook(plan, plan->d_cc_scratch)) != GL_OK) return rc;
    return gl::cc_finish(plan->d_cc_scratch, n, d_labels, d_count, "gl_cc_labels");
}
