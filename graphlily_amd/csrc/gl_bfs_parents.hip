// BFS predecessor tree from a finished level array (gl_bfs_parents): one pass over the rows of the plain CSR copy that every
// GL_PLAN_BOOLEAN plan keeps for the bottom-up BFS step (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base).
//
//   parent[v] = v            where level[v] == 1      (the source)
//             = 0xffffffff   where level[v] == 0      (not reached)
//             = min { u : A[v, u] != 0 and level[u] == level[v] - 1 }   otherwise (0xffffffff + one orphan if there is none)
//
// The result depends on the levels alone, not on the push / pull / bottom-up mix that produced them, so nothing in the step
// kernels or the recorded schedule changes.  Shape of the pass (EXPERIMENTS.md R7.*):
//   * the walk of gl_rows.h over every row that is searched; a row still undecided after `cut` entries is finished by the whole
//     wavefront with one butterfly min per row -- the stand-ins have rows of 1e5 entries;
//   * where every row's columns ascend (established once per plan, gl_rows.h: rows_sorted) the first
//     match is the minimum and the scan stops there; otherwise every entry is read;
//   * the levels are gathered from a one-byte copy (3 MB instead of 12 MB for 3 M vertices: it stays in the L2) that a
//     streaming pass packs first; a level array that does not fit a byte (>= 255, or not a whole number) raises a device flag
//     and the same launch gathers the floats instead -- no host decision, no synchronisation;
//   * entries with column 0xffffffff (zero-valued) are never parents.
#include "gl_rows.h"

#include <type_traits>

namespace gl {

constexpr uint32_t kNoParent = 0xffffffffu;
constexpr uint32_t kParentsCtlBytes = 256;   // scratch head: {u8 overflow flag, unsorted rows, orphans, -, entries read (64 bit)}

struct ParentsArgs {
    const uint32_t *row_ptr, *row_idx;
    const float *dist;
    const unsigned char *lev8;   // null: gather the floats
    const uint32_t *overflow;    // != 0: lev8 is not valid for this level array
    uint32_t *parent, *orphans;
    unsigned long long *reads;
    uint32_t row_begin, rows, num_cols, nz_base, cut_steps;
};

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m));
    return v;
}

// levels -> bytes, four per thread; anything a byte cannot hold exactly raises *overflow
__global__ __launch_bounds__(256) void parents_pack_levels_kernel(const float *__restrict__ d, uint32_t n, unsigned char *__restrict__ out,
                                                                  uint32_t *__restrict__ overflow) {
    bool bad = false;
    const uint32_t n4 = n >> 2;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        const float4 v = reinterpret_cast<const float4 *>(d)[i];
        const float f[4] = {v.x, v.y, v.z, v.w};
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t b = f[k] >= 0.0f && f[k] < 255.0f ? (uint32_t)f[k] : 255u;
            bad |= (float)b != f[k];
            w |= b << (8 * k);
        }
        reinterpret_cast<uint32_t *>(out)[i] = w;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) {
        const uint32_t i = (n4 << 2) + threadIdx.x;
        const float f = d[i];
        const uint32_t b = f >= 0.0f && f < 255.0f ? (uint32_t)f : 255u;
        bad |= (float)b != f;
        out[i] = (unsigned char)b;
    }
    if (__any(bad) && (threadIdx.x & 63u) == 0) atomicOr(overflow, 1u);
}

template <typename T, bool SORTED, bool COUNT>
__device__ __forceinline__ void parents_body(const ParentsArgs &a, const T *__restrict__ lev) {
    using W = typename std::conditional<std::is_same<T, float>::value, float, int>::type;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwords = (a.rows + 63u) >> 6;
    uint32_t orphans = 0;
    unsigned long long reads = 0;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += gridDim.x * 4u) {
        const uint32_t local = wd * 64u + lane;
        const bool in = local < a.rows;
        const uint32_t row = a.row_begin + local;
        const W lv = in ? (W)lev[row] : (W)0;
        const bool search = in && !(lv == (W)0) && !(lv == (W)1);
        const W want = lv - (W)1;
        uint32_t best = kNoParent, beg = 0, end = 0;
        if (search) {
            beg = a.row_ptr[local] - a.nz_base;
            end = a.row_ptr[local + 1u] - a.nz_base;
        }
        // (a row that is not searched keeps beg == end; on sorted rows the first match decides: the row is finished)
        rows_walk_thread(a.row_idx, beg, end, a.cut_steps, [&](const uint32_t(&c)[4], uint32_t at) {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c[u] < a.num_cols && (W)lev[c[u]] == want) best = min(best, c[u]);
            if (COUNT) reads += min(4u, end - at);
            return SORTED && best != kNoParent;
        });
        // rows still undecided: one butterfly min per row
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const W w = __shfl(want, src);
            uint32_t m = kNoParent;
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.num_cols && (W)lev[c[u]] == w) m = min(m, c[u]);
                if (COUNT && lane == 0) reads += min((uint64_t)256u, e - base);
                return SORTED && __any(m != kNoParent);
            });
            m = wave_min_u32(m);
            if ((int)lane == src) best = min(best, m);
        });
        if (in) a.parent[local] = lv == (W)0 ? kNoParent : lv == (W)1 ? row : best;
        orphans += search && best == kNoParent ? 1u : 0u;
    }
    if (__any(orphans != 0u)) atomicAdd(a.orphans, orphans);
    if (COUNT && __any(reads != 0ull)) atomicAdd(a.reads, reads);
}

template <bool SORTED, bool COUNT>
__global__ __launch_bounds__(256) void bfs_parents_kernel(ParentsArgs a) {
    if (a.lev8 != nullptr && *a.overflow == 0u)
        parents_body<unsigned char, SORTED, COUNT>(a, a.lev8);
    else
        parents_body<float, SORTED, COUNT>(a, a.dist);
}

// the refusals, the plan's scratch (control words + one byte per column) and its rows' sortedness, on first use
static int parents_prepare(gl_spmv_plan p, const char *who) {
    int rc = rows_require(p, kRowsIndexable, who, "the plan");
    if (rc == GL_OK) rc = plan_scratch(p->d_parents_scratch, kParentsCtlBytes + (((size_t)p->num_cols + 3u) & ~(size_t)3u), who, "level scratch");
    return rc == GL_OK ? rows_check_sorted(p) : rc;
}

static int parents_run(gl_spmv_plan p, const float *d_distance, uint32_t *d_parent, uint32_t *d_orphans, bool count, const char *who) {
    int rc = parents_prepare(p, who);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t rows = p->row_end - p->row_begin;
    uint32_t *ctl = reinterpret_cast<uint32_t *>(p->d_parents_scratch);
    unsigned char *lev8 = p->d_parents_scratch + kParentsCtlBytes;
    GL_HIP(hipMemsetAsync(ctl, 0, kParentsCtlBytes, s));
    if (d_orphans) GL_HIP(hipMemsetAsync(d_orphans, 0, 4, s));
    if (!rows) return GL_OK;
    // A/B knobs (GRAPHLILY_DEBUG, read per call): parents_cut = entries a thread reads before the wavefront takes the row
    // over, parents_grid = workgroups per compute unit, parents_u8 = 0 gathers the floats, parents_early = 0 takes the full-scan
    // path on sorted rows too
    const RowsWalkShape shape = rows_walk_shape(rows, debug_knob("parents_cut", 32), 1l << 30, debug_knob("parents_grid", 64));
    const bool u8 = debug_knob("parents_u8", 1) != 0 && ((uintptr_t)d_distance & 15u) == 0;
    const bool sorted = p->rows_sorted == 1 && debug_knob("parents_early", 1) != 0;
    if (u8) {
        const unsigned grid = std::max(1u, std::min<unsigned>((p->num_cols / 4u + 255u) / 256u, (unsigned)ctx().num_cus * 8u));
        parents_pack_levels_kernel<<<grid, 256, 0, s>>>(d_distance, p->num_cols, lev8, ctl);
        GL_LAUNCH_CHECK();
    }
    ParentsArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.dist = d_distance;
    a.lev8 = u8 ? lev8 : nullptr;
    a.overflow = ctl;
    a.parent = d_parent;
    a.orphans = d_orphans ? d_orphans : ctl + 2;
    a.reads = reinterpret_cast<unsigned long long *>(ctl + 4);
    a.row_begin = p->row_begin;
    a.rows = rows;
    a.num_cols = p->num_cols;
    a.nz_base = p->csr_nz_base;
    a.cut_steps = shape.cut_steps;
    const unsigned grid = shape.grid;
    if (sorted) {
        if (count) bfs_parents_kernel<true, true><<<grid, 256, 0, s>>>(a);
        else bfs_parents_kernel<true, false><<<grid, 256, 0, s>>>(a);
    } else {
        if (count) bfs_parents_kernel<false, true><<<grid, 256, 0, s>>>(a);
        else bfs_parents_kernel<false, false><<<grid, 256, 0, s>>>(a);
    }
    GL_LAUNCH_CHECK();
    return GL_OK;
}

}  // namespace gl

int gl_bfs_parents(gl_spmv_plan plan, const float *d_distance, uint32_t *d_parent, uint32_t *d_orphans) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_distance != nullptr && d_parent != nullptr);
    return gl::parents_run(plan, d_distance, d_parent, d_orphans, false, "gl_bfs_parents");
}

int gl_bfs_parents_entries(gl_spmv_plan plan, const float *d_distance, uint32_t *d_parent, uint64_t *entries_read) {
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_distance != nullptr && d_parent != nullptr && entries_read != nullptr);
    int rc = gl::parents_run(plan, d_distance, d_parent, nullptr, true, "gl_bfs_parents_entries");
    if (rc != GL_OK) return rc;
    hipStream_t s = gl::ctx().stream;
    uint64_t h = 0;
    const hipError_t e = hipMemcpyAsync(&h, plan->d_parents_scratch + 16, 8, hipMemcpyDeviceToHost, s);
    const hipError_t w = hipStreamSynchronize(s);
    GL_HIP(e != hipSuccess ? e : w);
    *entries_read = h;
    return GL_OK;
}
