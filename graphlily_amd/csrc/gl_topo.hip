// Topological levels and critical paths (gl_topo): Kahn's peeling of a directed graph with dependency counters, over the plain CSR
// copies that two GL_PLAN_BOOLEAN plans keep (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base) -- plan_in, whose row v
// lists the PREDECESSORS of v (an entry A[v, u] is an edge u -> v), and plan_out, the transposed pattern's plan, whose row v lists
// its SUCCESSORS (plan_out == plan_in: a symmetric pattern) -- on n = num_rows vertices.  An entry (v, v) is ignored.
//
//   level[v]  = the edges of the longest path that ends in v: 0 without predecessors, else 1 + max level[u] over the predecessors;
//               0xffffffff for a vertex on a cycle or reachable from one, which is never peeled
//   dist[v]   = (weights given) +0.0f for a peeled vertex without predecessors, else the largest, under > on float, of
//               (float)(dist[u] + w(u, v)) over the predecessors u; the bits 0x7fc00000 for an unpeeled vertex
//   parent[v] = the SMALLEST u that attains dist[v]; 0xffffffff for sources and unpeeled vertices
// All three are functions of (graph, weights): weights are finite and never -0.0 (the drivers see to both), so no candidate is NaN
// or -0.0 -- inf + finite is inf, x + (-x) is +0 -- and the monotone key of the f32 bits (gl_msf.hip's map) orders the candidates
// exactly as > does; the 64-bit word key(cand) << 32 | ~u, reduced by max, realises "largest candidate, then smallest u".
//
// STATE: pending[v] = the predecessors of v that are not peeled yet; a QUEUE of n words (d_order when the caller
// gives it), which a vertex enters exactly once, when its count reaches 0; a CONTROL RECORD {lo, hi, levels, widest, done} + tail
// (a line of its own: the only record word a round launch writes).
//   init   pending[v] = the length of row v of plan_in without the diagonal (one binary search: the rows ascend), level / dist /
//          parent = their unpeeled values, and every v whose count is 0 is appended: one ballot and one atomic add per wavefront
//   round  over the queue slice [lo, hi) fixed at launch, for every queued v:
//            level[v] = levels - 1, the number of the slice
//            PULL (weights given): one pass over row v of plan_in with its weights; dist[u] is read plainly -- every predecessor
//              was peeled in an earlier slice, so its dist was written by an earlier launch
//            PUSH: one pass over row v of plan_out: old = fetch_sub(pending[w], 1); old == 1: append w at tail  (once per vertex)
//          level[v], dist[v] and parent[v] have ONE writer, the owner of v: no float atomic, no spin-wait, no ticket
//   turn   (one thread)  lo = hi, hi = tail; a slice that is not empty is a level: levels += 1, widest = max(widest, hi - lo); an
//          empty one ends the run.  tail < n at the end is a RESULT -- the vertices left lie on a cycle or behind one -- where
//          color_turn_kernel reports an internal error.
// Both passes are the walk of gl_rows.h, a thread per queued vertex; the wavefront takes over a row still unfinished after
// topo_cut = 8 entries and reduces the pull's word across its lanes by shuffles; a wavefront that holds ONE vertex hands the rows to
// all its lanes at once (as color_round_kernel).  Every step issues its loads together, then its decrements, then its appends.
// MEMORY RULE and GATING: gl_rounds.h.  Atomic-only inside a round launch: pending[] and the tail.  The queue slice, the record,
// and the dist words a pull reads were written by earlier launches; level / dist / parent / queue words written now are read by
// later launches only.  The host enqueues (round, turn) x topo_batch; a launch that finds `done` returns at once.  Every round that
// runs peels a vertex, so at most n exist and the loop is capped at n + 1 steps; a batch that leaves the record as it was is an
// internal error.
#include "gl_rounds.h"
#include "graphlily_hip_topo.h"

namespace gl {

// the control record (words); the tail sits in the second 128-byte line
enum : uint32_t { kTopoLo = 0, kTopoHi = 1, kTopoLevels = 2, kTopoWidest = 3, kTopoDone = 4, kTopoRecordWords = 8, kTopoTail = 32 };
constexpr uint32_t kTopoNone = 0xffffffffu;      // the level and the parent of an unpeeled vertex, an unused queue word
constexpr uint32_t kTopoNaN = 0x7fc00000u;       // the dist bits of an unpeeled vertex

// gl_msf.hip's monotone map of the f32 bits to uint32, and its inverse
__device__ __forceinline__ uint32_t topo_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ uint32_t topo_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }
// the candidate of the predecessor u: larger distance first, then the SMALLER u.  Never 0: key 0 is the bits 0xffffffff, a NaN
__device__ __forceinline__ unsigned long long topo_word(float dist_u, float w, uint32_t u) {
    return ((unsigned long long)topo_key(__float_as_uint(dist_u + w)) << 32) | (uint32_t)~u;
}
__device__ __forceinline__ unsigned long long topo_shfl_xor(unsigned long long x, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}

struct TopoArgs {
    const uint32_t *in_ptr, *in_idx, *out_ptr, *out_idx;
    const float *weight;                           // NULL: no pull
    uint32_t *level, *parent, *pending, *queue, *ctl;
    float *dist;
    uint32_t n, in_base, out_base, cut_steps;
};

// the counters, the unpeeled values and the first slice's members; the record was zeroed by a memset in front of this launch
__global__ __launch_bounds__(256) void topo_init_kernel(TopoArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nround = ((uint64_t)a.n + 255u) & ~255ull;     // whole wavefronts take every trip
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < nround; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        const bool in = v64 < a.n;
        uint32_t count = 1u;
        if (in) {
            const uint32_t beg = a.in_ptr[v] - a.in_base, len = a.in_ptr[v + 1u] - a.in_base - beg;
            count = len;
            if (len != 0u && a.in_idx[beg + rows_lower_bound(a.in_idx + beg, len, v)] == v) count -= 1u;      // the diagonal
            a.pending[v] = count;                                 // (plain: nobody reads it in this launch)
            a.level[v] = kTopoNone;
            if (a.weight) {
                a.dist[v] = __uint_as_float(kTopoNaN);
                a.parent[v] = kTopoNone;
            }
        }
        const bool hit = in && count == 0u;
        const uint32_t pos = wave_append(hit, a.ctl + kTopoTail, lane);
        if (hit && pos < a.n) a.queue[pos] = v;                   // (pos < n: every vertex is appended once)
    }
}

// w's last predecessor has just been peeled (the decrement that returned 1): w joins the queue
__device__ __forceinline__ void topo_append(const TopoArgs &a, uint32_t w) {
    const uint32_t pos = ga_add(a.ctl + kTopoTail, 1u);
    if (pos < a.n) a.queue[pos] = w;
}

__global__ __launch_bounds__(256) void topo_round_kernel(TopoArgs a) {
    if (a.ctl[kTopoDone] != 0u) return;
    const uint32_t lo = a.ctl[kTopoLo], hi = a.ctl[kTopoHi], lvl = a.ctl[kTopoLevels] - 1u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t count = hi - lo, nwaves = gridDim.x * 4u;
    // queued vertices per wavefront: 64, fewer when the slice is shorter than the launch; a wavefront with ONE vertex gives its
    // rows to all lanes at once (color_round_kernel's dealing)
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    const uint32_t nwords = (uint32_t)(((uint64_t)count + per - 1u) / per);
    const uint32_t thread_steps = per == 1u ? 0u : a.cut_steps;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t item = (uint64_t)wd * per + lane;
        const bool in = lane < per && item < count;
        uint32_t v = kTopoNone, beg = 0, end = 0;
        if (in) {
            v = a.queue[lo + item];
            a.level[v] = lvl;
        }
        if (a.weight) {                                           // PULL: the best candidate over row v of plan_in
            if (in) {
                beg = a.in_ptr[v] - a.in_base;
                end = a.in_ptr[v + 1u] - a.in_base;
            }
            unsigned long long best = 0ull;                       // (no candidate is 0)
            rows_walk_thread(a.in_idx, beg, end, thread_steps, [&](const uint32_t(&c)[4], uint32_t at) {
                float w[4], d[4];
#pragma unroll
                for (int u = 0; u < 4; u++) w[u] = end - at > (uint32_t)u ? a.weight[at + u] : 0.0f;
#pragma unroll
                for (int u = 0; u < 4; u++) d[u] = (c[u] < a.n && c[u] != v) ? a.dist[c[u]] : 0.0f;
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n && c[u] != v) best = max(best, topo_word(d[u], w[u], c[u]));
                return false;
            });
            rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
                const uint32_t row = __shfl(v, src);
                unsigned long long m = (int)lane == src ? best : 0ull;       // (what its own thread found joins the maximum)
                rows_walk_wave(a.in_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
                    float w[4], d[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint64_t j = base + 64u * u + lane;
                        w[u] = j < e ? a.weight[j] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) d[u] = (c[u] < a.n && c[u] != row) ? a.dist[c[u]] : 0.0f;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (c[u] < a.n && c[u] != row) m = max(m, topo_word(d[u], w[u], c[u]));
                    return false;
                });
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) m = max(m, topo_shfl_xor(m, d));
                if ((int)lane == src) best = m;
            });
            if (in) {
                a.dist[v] = best ? __uint_as_float(topo_unkey((uint32_t)(best >> 32))) : 0.0f;
                a.parent[v] = best ? ~(uint32_t)best : kTopoNone;
            }
        }
        beg = end = 0u;                                           // PUSH: release the successors of v
        if (in) {
            beg = a.out_ptr[v] - a.out_base;
            end = a.out_ptr[v + 1u] - a.out_base;
        }
        rows_walk_thread(a.out_idx, beg, end, thread_steps, [&](const uint32_t(&c)[4], uint32_t) {
            uint32_t old[4];
#pragma unroll
            for (int u = 0; u < 4; u++) old[u] = (c[u] < a.n && c[u] != v) ? ga_sub(a.pending + c[u], 1u) : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (old[u] == 1u) topo_append(a, c[u]);
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t row = __shfl(v, src);
            rows_walk_wave(a.out_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                uint32_t old[4];
#pragma unroll
                for (int u = 0; u < 4; u++) old[u] = (c[u] < a.n && c[u] != row) ? ga_sub(a.pending + c[u], 1u) : 0u;
#pragma unroll
                for (int u = 0; u < 4; u++) {                     // (every lane is here: one atomic add per wavefront and step)
                    const bool hit = old[u] == 1u;
                    const uint32_t pos = wave_append(hit, a.ctl + kTopoTail, lane);
                    if (hit && pos < a.n) a.queue[pos] = c[u];
                }
                return false;
            });
        });
    }
}

// behind a round (or init): plain loads and stores, a launch of its own
__global__ void topo_turn_kernel(uint32_t *ctl, uint32_t n) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    if (ctl[kTopoDone] != 0u) return;
    const uint32_t lo = ctl[kTopoHi], hi = min(ctl[kTopoTail], n);
    ctl[kTopoLo] = lo;
    ctl[kTopoHi] = hi;
    if (hi == lo) {
        ctl[kTopoDone] = 1u;                                      // (hi < n: what is left lies on a cycle or behind one)
    } else {
        ctl[kTopoLevels] += 1u;
        ctl[kTopoWidest] = max(ctl[kTopoWidest], hi - lo);
    }
}

// a graph without entries: every vertex is a source of level 0
__global__ __launch_bounds__(256) void topo_flat_kernel(uint32_t *__restrict__ level, uint32_t *__restrict__ order, float *__restrict__ dist,
                                                        uint32_t *__restrict__ parent, uint32_t n) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        level[v] = 0u;
        if (order) order[v] = (uint32_t)v;
        if (dist) dist[v] = 0.0f;
        if (parent) parent[v] = kTopoNone;
    }
}

// the words of plan_in's scratch: the control record, pending, the queue
constexpr size_t topo_scratch_bytes(size_t n) { return kRoundsCtlBytes + 8u * n; }

static int topo(gl_spmv_plan pin, gl_spmv_plan pout, const float *d_weight, uint32_t *d_level, uint32_t *d_order, float *d_dist,
                uint32_t *d_parent, uint64_t *h_stats, const char *who) {
    int rc = rows_require_pair(pin, pout, who, "io.simple_pattern");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = pin->num_rows;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0u;
    if (n == 0u) return GL_OK;
    // the outputs are distinct arrays of n words, and none of them is the weights
    {
        const void *out[4] = {d_level, d_order, d_dist, d_parent};
        const size_t bytes = 4u * (size_t)n, wbytes = 4u * (size_t)pin->nnz;
        for (int i = 0; i < 4; i++) {
            if (!out[i]) continue;
            const char *p = (const char *)out[i], *w = (const char *)d_weight;
            if (w && wbytes && p < w + wbytes && w < p + bytes) return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: an output array overlaps d_weight", who);
            for (int j = i + 1; j < 4; j++) {
                const char *q = (const char *)out[j];
                if (q && p < q + bytes && q < p + bytes) return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: two output arrays overlap", who);
            }
        }
    }
    const unsigned stream_grid = rows_stream_grid(n);
    if (pin->nnz == 0) {                                          // no entries: one level holds everybody
        topo_flat_kernel<<<stream_grid, 256, 0, s>>>(d_level, d_order, d_dist, d_parent, n);
        GL_LAUNCH_CHECK();
        GL_HIP(hipStreamSynchronize(s));
        if (h_stats) {
            h_stats[0] = h_stats[2] = n;
            h_stats[1] = h_stats[3] = 1u;
        }
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 28): topo_cut = entries a thread reads of a row before the
    // wavefront takes it over, topo_grid = workgroups per compute unit of a round launch, topo_batch = (round, turn) pairs
    // enqueued between two read-backs of the control record.  gl_color's values, as starting values.
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("topo_cut", 8), 1l << 30, debug_knob("topo_grid", 4));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("topo_batch", 64), 4096));
    rc = plan_scratch(pin->d_topo_scratch, topo_scratch_bytes(n), who, "control record, counters and queue");
    if (rc != GL_OK) return rc;
    TopoArgs a;
    a.in_ptr = pin->d_csr_indptr;
    a.in_idx = pin->d_csr_indices;
    a.in_base = pin->csr_nz_base;
    a.out_ptr = pout->d_csr_indptr;
    a.out_idx = pout->d_csr_indices;
    a.out_base = pout->csr_nz_base;
    a.weight = d_weight;
    a.level = d_level;
    a.dist = d_dist;
    a.parent = d_parent;
    a.ctl = reinterpret_cast<uint32_t *>(pin->d_topo_scratch);
    a.pending = a.ctl + kRoundsCtlBytes / 4u;
    a.queue = d_order ? d_order : a.pending + n;
    a.n = n;
    a.cut_steps = shape.cut_steps;
    const unsigned round_grid = shape.grid;
    static_assert((kTopoRecordWords + 1u) * 4u <= 64u, "the record and the tail fit the page-locked staging words");
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    uint32_t seen[kTopoRecordWords + 1u];                         // the record as the batch before left it
    for (uint32_t i = 0; i <= kTopoRecordWords; i++) seen[i] = w[i] = 0u;
    GL_HIP(hipMemsetAsync(a.ctl, 0, kRoundsCtlBytes, s));
    if (d_order) GL_HIP(hipMemsetAsync(d_order, 0xff, 4u * (size_t)n, s));      // the words behind the peeled vertices
    topo_init_kernel<<<stream_grid, 256, 0, s>>>(a);
    topo_turn_kernel<<<1, 64, 0, s>>>(a.ctl, n);
    GL_LAUNCH_CHECK();
    uint64_t launches = 2;
    bool stuck = false;
    rc = rounds_run(
        batch, (uint64_t)n + 1ull, launches,                      // every round that runs peels a vertex
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                topo_round_kernel<<<round_grid, 256, 0, s>>>(a);
                topo_turn_kernel<<<1, 64, 0, s>>>(a.ctl, n);
            }
            return 2ull * batch;
        },
        [&] {
            const hipError_t e = hipMemcpyAsync(w, a.ctl, kTopoRecordWords * 4u, hipMemcpyDeviceToHost, s);
            return e != hipSuccess ? e : hipMemcpyAsync(w + kTopoRecordWords, a.ctl + kTopoTail, 4u, hipMemcpyDeviceToHost, s);
        },
        [&] {
            if (w[kTopoDone] != 0u) return kRoundsDone;
            stuck = true;
            for (uint32_t i = 0; i <= kTopoRecordWords; i++) {
                stuck = stuck && seen[i] == w[i];
                seen[i] = w[i];
            }
            return stuck ? kRoundsStuck : kRoundsGoOn;
        },
        [&](uint64_t steps) {
            return set_error(GL_ERR_HIP, "%s: internal error: %s after %llu steps on %u vertices (%u levels, %u vertices queued)", who,
                             stuck ? "a batch did not move the control record" : "not done", (unsigned long long)steps, n, w[kTopoLevels],
                             w[kTopoRecordWords]);
        });
    if (rc != GL_OK) return rc;
    if (h_stats) {
        h_stats[0] = w[kTopoHi];
        h_stats[1] = w[kTopoLevels];
        h_stats[2] = w[kTopoWidest];
        h_stats[3] = launches;
    }
    return GL_OK;
}

}  // namespace gl

int gl_topo(gl_spmv_plan plan_in, gl_spmv_plan plan_out, const float *d_weight, uint32_t *d_level, uint32_t *d_order, float *d_dist,
            uint32_t *d_parent, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan_in != nullptr && plan_out != nullptr && d_level != nullptr);
    GL_ARG((d_weight != nullptr) == (d_dist != nullptr) && (d_weight != nullptr) == (d_parent != nullptr));
    return gl::topo(plan_in, plan_out, d_weight, d_level, d_order, d_dist, d_parent, h_stats, "gl_topo");
}
