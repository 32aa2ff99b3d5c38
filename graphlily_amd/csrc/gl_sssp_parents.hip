// Shortest-path predecessor tree from a finished distance array (gl_sssp_parents): one pass over the CSC stream that every
// SpMSpV plan keeps (gl_spmspv.hip: d_indptr, num_cols + 1 offsets, and d_stream of {global row, value bits}).
//
//   parent[s] = s
//   parent[v] = 0xffffffff                        where d[v] >= unreached
//   parent[v] = min { u : A[v,u] stored with weight w, d[u] < d[v] and (float)(d[u] + w) == d[v] }   otherwise
//               (0xffffffff + one orphan if there is no such u)
//
// General SpMV plans keep no plain weighted rows, the CSC plan of the drivers does, so the pass walks COLUMNS and scatters:
// column u (skipped when d[u] >= unreached) issues atomicMin(&parent[v], u) for each of its entries (v, w) that is tight.
// min is order-independent, so the result is unique whatever the order of arrival; the atomic's return value is not used.
// d[u] < d[v] is strict: no cycles through weight-0 or absorbed (d + w == d) entries, and never the weight-0 self edges.
// Shape: gl_bfs_parents.hip turned on its side --
//   * 64 columns per wavefront, a thread per column, four entries per step; d[u] is uniform per column, d[v] is the one
//     random 4-byte gather per entry;
//   * a column still unfinished after `cut` entries is taken over by the whole wavefront, 256 entries per step with
//     coalesced 8-byte loads -- the stand-ins have columns of 1e5 entries;
//   * nothing stops early: every entry of a reached column is read;
//   * around it, on the library's stream: parent is filled with 0xffffffff first, and a finish pass over the shard's rows
//     stores parent[source] = source and counts the orphans.  No host synchronisation.
#include "gl_spmv_plan.h"

namespace gl {

constexpr uint32_t kSsspNoParent = 0xffffffffu;
constexpr uint32_t kSsspCtlBytes = 32;   // {orphans, -, entries read (64 bit), -}

struct SsspParentsArgs {
    const uint32_t *indptr;
    const uint2 *stream;
    const float *dist;
    uint32_t *parent;            // the shard's rows: parent[v - row_begin]
    unsigned long long *reads;
    uint32_t row_begin, num_cols, cut_steps;
    float unreached;
};

// entry (v, w) of a column whose vertex u has distance du: is u -> v a tree-edge candidate?  (v is a row of the shard and
// num_rows <= num_cols, so dist[v] exists)
__device__ __forceinline__ void sssp_relax_check(const SsspParentsArgs &a, uint2 e, float du, uint32_t u) {
    const float dv = a.dist[e.x];
    if (du < dv && dv < a.unreached && du + __uint_as_float(e.y) == dv) atomicMin(a.parent + (e.x - a.row_begin), u);
}

template <bool COUNT>
__global__ __launch_bounds__(256) void sssp_parents_scatter_kernel(SsspParentsArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwords = (a.num_cols + 63u) >> 6;
    unsigned long long reads = 0;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += gridDim.x * 4u) {
        const uint32_t col = wd * 64u + lane;
        const bool in = col < a.num_cols;
        const float du = in ? a.dist[col] : a.unreached;
        const bool live = in && du < a.unreached;
        uint32_t beg = 0, end = 0;
        if (live) {
            beg = a.indptr[col];
            end = a.indptr[col + 1u];
        }
        if (COUNT) reads += end - beg;
        for (uint32_t step = 0; step < a.cut_steps && __any(beg < end); step++) {
            if (beg < end) {
                uint2 e[4];
#pragma unroll
                for (int k = 0; k < 4; k++) e[k] = beg + k < end ? a.stream[beg + k] : make_uint2(0u, 0u);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (beg + k < end) sssp_relax_check(a, e[k], du, col);
                beg += 4u;
            }
        }
        // columns still unfinished are read by the whole wavefront, 256 entries per step (coalesced 8-byte loads)
        for (uint64_t pending = __ballot(beg < end); pending; pending &= pending - 1ull) {
            const int src = __ffsll((unsigned long long)pending) - 1;
            const uint32_t b = __shfl(beg, src), e = __shfl(end, src), u = __shfl(col, src);
            const float d = __shfl(du, src);
            for (uint32_t base = b; base < e; base += 256u) {
                uint2 r[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t i = base + 64u * k + lane;
                    r[k] = i < e ? load_stream_nt(a.stream + i) : make_uint2(0u, 0u);
                }
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (base + 64u * k + lane < e) sssp_relax_check(a, r[k], d, u);
            }
        }
    }
    if (COUNT && __any(reads != 0ull)) atomicAdd(a.reads, reads);
}

// after the scatter: the source is its own parent whatever the scatter left there, and a reached row without a parent is
// an orphan
__global__ __launch_bounds__(256) void sssp_parents_finish_kernel(const float *__restrict__ dist, uint32_t *__restrict__ parent, uint32_t row_begin,
                                                                  uint32_t rows, uint32_t source, float unreached, uint32_t *__restrict__ orphans) {
    uint32_t n = 0;
    for (uint32_t local = blockIdx.x * 256u + threadIdx.x; local < rows; local += gridDim.x * 256u) {
        const uint32_t v = row_begin + local;
        if (v == source)
            parent[local] = source;
        else if (dist[v] < unreached && parent[local] == kSsspNoParent)
            n++;
    }
    if (__any(n != 0u)) atomicAdd(orphans, n);
}

static int sssp_parents_run(gl_spmspv_plan plan, const float *d_distance, float unreached, uint32_t source, uint32_t *d_parent,
                            uint32_t *d_orphans, bool count, const char *who) {
    const SpmspvCsc c = spmspv_plan_csc(plan);
    if (source >= c.num_cols) return set_error(GL_ERR_INVALID_ARG, "%s: source %u of %u vertices", who, source, c.num_cols);
    if (c.row_end > c.num_cols)
        return set_error(GL_ERR_UNSUPPORTED, "%s: the distance vector is indexed by row and by column: needs num_rows <= num_cols", who);
    hipStream_t s = ctx().stream;
    if (!*c.ctl) {
        hipError_t e = hipMalloc((void **)c.ctl, kSsspCtlBytes);
        if (e != hipSuccess) return set_error(GL_ERR_HIP, "%s: hipMalloc(%u bytes of control words): %s", who, kSsspCtlBytes, hipGetErrorString(e));
    }
    uint32_t *ctl = *c.ctl;
    const uint32_t rows = c.row_end - c.row_begin;
    GL_HIP(hipMemsetAsync(ctl, 0, kSsspCtlBytes, s));
    if (d_orphans) GL_HIP(hipMemsetAsync(d_orphans, 0, 4, s));
    if (!rows) return GL_OK;
    GL_HIP(hipMemsetAsync(d_parent, 0xff, (size_t)rows * 4u, s));
    // A/B knobs (GRAPHLILY_DEBUG, read per call): sssp_parents_cut = entries a thread reads before the wavefront takes the
    // column over, sssp_parents_grid = workgroups per compute unit
    const long cut = debug_knob("sssp_parents_cut", 32);
    SsspParentsArgs a;
    a.indptr = c.indptr;
    a.stream = c.stream;
    a.dist = d_distance;
    a.parent = d_parent;
    a.reads = reinterpret_cast<unsigned long long *>(ctl + 2);
    a.row_begin = c.row_begin;
    a.num_cols = c.num_cols;
    a.cut_steps = (uint32_t)std::max<long>(0, std::min<long>(cut, 1l << 30)) / 4u;
    a.unreached = unreached;
    const unsigned per_cu = (unsigned)std::max<long>(1, std::min<long>(debug_knob("sssp_parents_grid", 64), 1024));
    const unsigned nwords = (c.num_cols + 63u) / 64u;
    const unsigned grid = std::max(1u, std::min<unsigned>((nwords + 3u) / 4u, (unsigned)ctx().num_cus * per_cu));
    if (count) sssp_parents_scatter_kernel<true><<<grid, 256, 0, s>>>(a);
    else sssp_parents_scatter_kernel<false><<<grid, 256, 0, s>>>(a);
    GL_LAUNCH_CHECK();
    const unsigned fgrid = std::max(1u, std::min<unsigned>((rows + 255u) / 256u, (unsigned)ctx().num_cus * 8u));
    sssp_parents_finish_kernel<<<fgrid, 256, 0, s>>>(d_distance, d_parent, c.row_begin, rows, source, unreached, d_orphans ? d_orphans : ctl);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl

int gl_sssp_parents(gl_spmspv_plan plan, const float *d_distance, float unreached, uint32_t source, uint32_t *d_parent, uint32_t *d_orphans) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_distance != nullptr && d_parent != nullptr);
    return gl::sssp_parents_run(plan, d_distance, unreached, source, d_parent, d_orphans, false, "gl_sssp_parents");
}

int gl_sssp_parents_entries(gl_spmspv_plan plan, const float *d_distance, float unreached, uint32_t source, uint32_t *d_parent,
                            uint64_t *entries_read) {
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_distance != nullptr && d_parent != nullptr && entries_read != nullptr);
    int rc = gl::sssp_parents_run(plan, d_distance, unreached, source, d_parent, nullptr, true, "gl_sssp_parents_entries");
    if (rc != GL_OK) return rc;
    hipStream_t s = gl::ctx().stream;
    uint64_t h = 0;
    const hipError_t e = hipMemcpyAsync(&h, *gl::spmspv_plan_csc(plan).ctl + 2, 8, hipMemcpyDeviceToHost, s);
    const hipError_t w = hipStreamSynchronize(s);
    GL_HIP(e != hipSuccess ? e : w);
    *entries_read = h;
    return GL_OK;
}
