// Bit-parallel multi-source breadth-first search (gl_msbfs; Then et al., "The More the Merrier", VLDB 2014): up to 64 searches
// share one sweep over the plain CSR copy that a GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices /
// csr_nz_base), on n = num_rows vertices.  An entry A[v, u] is an edge u -> v, so row v lists the PREDECESSORS of v; a column
// 0xffffffff (a zero-valued entry) is no edge, a diagonal entry is harmless.  d(s, v) = the edges of a shortest path from s to v.
//
//   far[v]      = the sum of d(s, v) over the sources s with 1 <= d(s, v) < inf          (u64)
//   reach[v]    = the number of those sources                                            (u32)
//   harmonic[v] = the f64 sum of (double)c / (double)d over the levels d = 1, 2, ... ASCENDING, c = the sources that reach v at
//                 level d: one division and one addition per level with c > 0, by the owner of v -- no floating-point atomic
//   hops[j n + v] = d(source j, v): 0 on the source, 0xffffffff when unreached            (optional)
// With `accumulate` the first three are added to, otherwise the begin kernel zeroes them.
//
// STATE: every vertex holds 64-bit words with one bit per source -- seen[v] (the sources that have met v) and two
// frontier buffers selected by the level's parity; a level d is
//     next[v] = (OR over the u of row v of front[u]) & ~seen[v],     seen[v] |= next[v]
// with front = buffer (d - 1) & 1 and next = buffer d & 1.  Every vertex has ONE writer, its owner, and front was written by an
// earlier launch: seen[], the frontiers, far / reach / harmonic / hops are PLAIN words behind launch boundaries.
//   begin  seen[v] = front0[v] = the bits of the sources that are v (a source given twice holds two bits), the outputs' initial
//          values, every word of hops
//   level  (d = the launch's own argument: one launch per level) a thread per row -- the walk of gl_rows.h, the wavefront taking
//          over a row still unfinished after msbfs_cut entries and reducing the word across its lanes by shuffles.  A row whose
//          seen equals the k-bit mask (the LOW k bits) reads no index and writes next[v] = 0; a body stops as soon as acc | seen
//          equals the mask.  The owner writes next, and for new bits seen, far, reach, harmonic and hops.  The new bits are counted
//          per source in LDS (64 counters per workgroup) and go to the global counters with one integer atomic per non-zero
//          counter and workgroup.
// MEMORY RULE and GATING: gl_rounds.h.  Atomic-only (ga_*) inside a level launch: the two control words -- `last`, the largest
// level that added a bit (ga_max by the workgroups that added one, ga_load by the gate), and `full`, the vertices that have met all
// k sources -- and the per-source counters {reach, far, eccentricity} x 64.  A launch of level d returns at once unless last >=
// d - 1: the level before it added no bit, and then no later one does, so `last` stays and every later launch returns too.  The
// host enqueues msbfs_batch levels blindly and reads `last` back once per batch; last < the last level enqueued means done, and
// the result does not depend on the batch.  A level that adds a bit lengthens a shortest path, which has at most n - 1 edges, so
// level n adds nothing and the loop is capped at n + 1 steps.
#include "gl_rounds.h"
#include "graphlily_hip_msbfs.h"

namespace gl {

// the control words (the second 128-byte line: level launches add to them), then the per-source counters behind the record
enum : uint32_t { kMsbfsLast = 32, kMsbfsFull = 33 };
constexpr uint32_t kMsbfsNone = 0xffffffffu;             // the hops of an unreached vertex
constexpr size_t kMsbfsCounterBytes = 64u * 8u + 64u * 8u + 64u * 4u;      // reach (u64), far (u64), eccentricity (u32)
constexpr size_t msbfs_scratch_bytes(size_t n) { return kRoundsCtlBytes + kMsbfsCounterBytes + 24u * n; }

__device__ __forceinline__ unsigned long long msbfs_shfl(unsigned long long x, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long msbfs_shfl_xor(unsigned long long x, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}

struct MsbfsArgs {
    const uint32_t *row_ptr, *row_idx;
    unsigned long long *seen, *front[2], *far, *cnt_reach, *cnt_far;
    uint32_t *reach, *hops, *ctl, *cnt_ecc;
    double *harmonic;
    unsigned long long mask;
    uint32_t n, nz_base, k, cut_steps, accumulate;
};
struct MsbfsSources {
    uint32_t v[64];
};

__global__ __launch_bounds__(256) void msbfs_begin_kernel(MsbfsArgs a, MsbfsSources src) {
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < a.n; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        unsigned long long word = 0ull;
        for (uint32_t j = 0; j < a.k; j++) word |= src.v[j] == v ? 1ull << j : 0ull;
        a.seen[v] = word;
        a.front[0][v] = word;
        if (!a.accumulate) {
            a.far[v] = 0ull;
            a.reach[v] = 0u;
            a.harmonic[v] = 0.0;
        }
        if (a.hops)
            for (uint32_t j = 0; j < a.k; j++) a.hops[(size_t)j * a.n + v] = (word >> j) & 1ull ? 0u : kMsbfsNone;
        if (word == a.mask) (void)ga_add(a.ctl + kMsbfsFull, 1u);           // (all k sources are this vertex)
    }
}

__global__ __launch_bounds__(256) void msbfs_level_kernel(MsbfsArgs a, uint32_t d) {
    if (ga_load(a.ctl + kMsbfsLast) + 1u < d) return;              // the level before this one added no bit
    __shared__ uint32_t s_cnt[64], s_full;
    if (threadIdx.x < 64u) s_cnt[threadIdx.x] = 0u;
    if (threadIdx.x == 64u) s_full = 0u;
    __syncthreads();
    const unsigned long long *__restrict__ front = d & 1u ? a.front[0] : a.front[1];       // (selected, not indexed: the
    unsigned long long *__restrict__ next = d & 1u ? a.front[1] : a.front[0];              // arguments stay in registers)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * 4u, nwords = (uint32_t)(((uint64_t)a.n + 63u) / 64u);
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t v64 = (uint64_t)wd * 64u + lane;
        const uint32_t v = (uint32_t)v64;
        const bool in = v64 < a.n;
        const unsigned long long seen = in ? a.seen[v] : a.mask;
        const bool live = seen != a.mask;                          // a row that has met all its sources reads no index
        uint32_t beg = 0, end = 0;
        if (live) {
            beg = a.row_ptr[v] - a.nz_base;
            end = a.row_ptr[v + 1u] - a.nz_base;
        }
        unsigned long long acc = 0ull;
        rows_walk_thread(a.row_idx, beg, end, a.cut_steps, [&](const uint32_t(&c)[4], uint32_t) {
            unsigned long long f[4];
#pragma unroll
            for (int u = 0; u < 4; u++) f[u] = c[u] < a.n ? front[c[u]] : 0ull;
            acc |= (f[0] | f[1]) | (f[2] | f[3]);
            return (acc | seen) == a.mask;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const unsigned long long row_seen = msbfs_shfl(seen, src);
            unsigned long long m = msbfs_shfl(acc, src);           // what its own thread found, in every lane
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                unsigned long long f[4];
#pragma unroll
                for (int u = 0; u < 4; u++) f[u] = c[u] < a.n ? front[c[u]] : 0ull;
                m |= (f[0] | f[1]) | (f[2] | f[3]);
#pragma unroll
                for (int x = 1; x < 64; x <<= 1) m |= msbfs_shfl_xor(m, x);      // the same word in every lane
                return (m | row_seen) == a.mask;
            });
            if ((int)lane == src) acc = m;
        });
        if (in) {
            const unsigned long long fresh = acc & ~seen;
            next[v] = fresh;
            if (fresh != 0ull) {
                const uint32_t c = (uint32_t)__popcll(fresh);
                a.seen[v] = seen | fresh;
                a.far[v] += (unsigned long long)c * d;
                a.reach[v] += c;
                a.harmonic[v] = a.harmonic[v] + (double)c / (double)d;
                for (unsigned long long w = fresh; w; w &= w - 1ull) {
                    const uint32_t j = (uint32_t)__ffsll(w) - 1u;
                    atomicAdd(&s_cnt[j], 1u);
                    if (a.hops) a.hops[(size_t)j * a.n + v] = d;
                }
                if ((seen | fresh) == a.mask) atomicAdd(&s_full, 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64u) {
        const uint32_t c = s_cnt[threadIdx.x];
        if (c != 0u) {
            ga_add(a.cnt_reach + threadIdx.x, (unsigned long long)c);
            ga_add(a.cnt_far + threadIdx.x, (unsigned long long)c * d);
            ga_max(a.cnt_ecc + threadIdx.x, d);
        }
        if (__ballot(c != 0u) != 0ull && threadIdx.x == 0u) ga_max(a.ctl + kMsbfsLast, d);
    }
    if (threadIdx.x == 64u && s_full != 0u) (void)ga_add(a.ctl + kMsbfsFull, s_full);
}

static int msbfs(gl_spmv_plan p, const uint32_t *h_sources, uint32_t k, int accumulate, uint64_t *d_far, uint32_t *d_reach,
                 double *d_harmonic, uint32_t *d_hops, uint64_t *h_source_stats, uint64_t *h_stats, const char *who) {
    int rc = rows_require(p, kRowsSquare, who, "the plan");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_rows;
    if (n == 0u) return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: a plan without vertices has no source to name", who);
    MsbfsSources src;
    for (uint32_t j = 0; j < 64u; j++) src.v[j] = kMsbfsNone;
    for (uint32_t j = 0; j < k; j++) {
        if (h_sources[j] >= n)
            return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: source %u is vertex %u of %u", who, j, h_sources[j], n);
        src.v[j] = h_sources[j];
    }
    {
        const void *out[4] = {d_far, d_reach, d_harmonic, d_hops};
        const size_t bytes[4] = {8u * (size_t)n, 4u * (size_t)n, 8u * (size_t)n, 4u * (size_t)n * k};
        for (int i = 0; i < 4; i++) {
            const char *x = (const char *)out[i];
            for (int j = i + 1; x && j < 4; j++) {
                const char *y = (const char *)out[j];
                if (y && x < y + bytes[j] && y < x + bytes[i])
                    return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: two output arrays overlap", who);
            }
        }
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 29): msbfs_cut = entries a thread reads of a row before the
    // wavefront takes it over, msbfs_grid = workgroups per compute unit of a level launch, msbfs_batch = levels enqueued between
    // two read-backs of the control words
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("msbfs_cut", 8), 1l << 30, debug_knob("msbfs_grid", 4));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("msbfs_batch", 16), 4096));
    rc = plan_scratch(p->d_msbfs_scratch, msbfs_scratch_bytes(n), who, "control record, counters, seen words and two frontiers");
    if (rc != GL_OK) return rc;
    MsbfsArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.nz_base = p->csr_nz_base;
    a.ctl = reinterpret_cast<uint32_t *>(p->d_msbfs_scratch);
    a.cnt_reach = reinterpret_cast<unsigned long long *>(p->d_msbfs_scratch + kRoundsCtlBytes);
    a.cnt_far = a.cnt_reach + 64;
    a.cnt_ecc = reinterpret_cast<uint32_t *>(a.cnt_far + 64);
    a.seen = reinterpret_cast<unsigned long long *>(p->d_msbfs_scratch + kRoundsCtlBytes + kMsbfsCounterBytes);
    a.front[0] = a.seen + n;
    a.front[1] = a.front[0] + n;
    a.far = reinterpret_cast<unsigned long long *>(d_far);
    a.reach = d_reach;
    a.harmonic = d_harmonic;
    a.hops = d_hops;
    a.mask = k == 64u ? ~0ull : (1ull << k) - 1ull;
    a.n = n;
    a.k = k;
    a.cut_steps = shape.cut_steps;
    a.accumulate = accumulate ? 1u : 0u;
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    w[0] = w[1] = 0u;
    GL_HIP(hipMemsetAsync(a.ctl, 0, kRoundsCtlBytes + kMsbfsCounterBytes, s));
    msbfs_begin_kernel<<<rows_stream_grid(n), 256, 0, s>>>(a, src);
    GL_LAUNCH_CHECK();
    uint64_t launches = 1;
    uint32_t level = 0;                                           // the last level enqueued
    if (p->nnz == 0) {                                            // no entries: the begin kernel has answered
        GL_HIP(hipMemcpyAsync(w, a.ctl + kMsbfsLast, 8u, hipMemcpyDeviceToHost, s));
        GL_HIP(hipStreamSynchronize(s));
    } else {
        rc = rounds_run(
            batch, (uint64_t)n + 1ull, launches,                  // a level that adds a bit lengthens a shortest path
            [&] {
                for (uint32_t i = 0; i < batch; i++) msbfs_level_kernel<<<shape.grid, 256, 0, s>>>(a, ++level);
                return (uint64_t)batch;
            },
            [&] { return hipMemcpyAsync(w, a.ctl + kMsbfsLast, 8u, hipMemcpyDeviceToHost, s); },
            [&] { return w[0] < level ? kRoundsDone : kRoundsGoOn; },
            [&](uint64_t steps) {
                return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu steps on %u vertices (level %u added a bit)", who,
                                 (unsigned long long)steps, n, w[0]);
            });
        if (rc != GL_OK) return rc;
    }
    if (h_stats) {
        h_stats[0] = w[0];
        h_stats[1] = w[1];
        h_stats[2] = launches;
        h_stats[3] = 0u;
    }
    if (h_source_stats) {
        uint64_t cnt[kMsbfsCounterBytes / 8u];
        const hipError_t e = hipMemcpyAsync(cnt, a.cnt_reach, kMsbfsCounterBytes, hipMemcpyDeviceToHost, s);
        const hipError_t e2 = hipStreamSynchronize(s);            // (waited for either way: cnt is a stack array)
        GL_HIP(e);
        GL_HIP(e2);
        const uint32_t *ecc = reinterpret_cast<const uint32_t *>(cnt + 128);
        for (uint32_t j = 0; j < k; j++) {
            h_source_stats[3u * j] = cnt[j];
            h_source_stats[3u * j + 1u] = cnt[64u + j];
            h_source_stats[3u * j + 2u] = ecc[j];
        }
    }
    return GL_OK;
}

}  // namespace gl

int gl_msbfs(gl_spmv_plan plan, const uint32_t *h_sources, uint32_t k, int accumulate, uint64_t *d_far, uint32_t *d_reach,
             double *d_harmonic, uint32_t *d_hops, uint64_t *h_source_stats, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && h_sources != nullptr);
    GL_ARG(d_far != nullptr && d_reach != nullptr && d_harmonic != nullptr);
    GL_ARG(k >= 1u && k <= 64u);
    return gl::msbfs(plan, h_sources, k, accumulate, d_far, d_reach, d_harmonic, d_hops, h_source_stats, h_stats, "gl_msbfs");
}
