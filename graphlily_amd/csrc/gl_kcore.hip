// k-core decomposition (gl_kcore): level-synchronous peeling (PKC-style, after Kabir & Madduri) over the plain CSR copy
// that every GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base), on a square, whole-matrix
// plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is SYMMETRIC, over n = num_rows
// vertices.  An entry (v, v) is ignored.
//
//   core[v]  = the largest k such that v lies in a subgraph in which every vertex has degree >= k (isolated vertices: 0)
//   order    = (optional) a permutation of the vertices in which core[order[i]] never descends and every vertex has at most
//              core[v] neighbours behind it: the order in which the vertices were peeled.  Not unique.
//
// STATE: deg[n], which IS d_core -- a vertex's degree is frozen at the level it is peeled at, so the array ends
// up as the core numbers; a QUEUE of n words (d_order, or plan-owned scratch), which every vertex enters exactly once; and a
// CONTROL RECORD {k, lo, hi, phase, counters} + tail (a line of its own).  No "alive" array: peeled vertices have deg <= k - 1,
// or == k once they are queued at this level.
//   scan   (phase "scan")  appends every v with deg[v] == k: one ballot and one atomic add to tail per wavefront
//   peel   (phase "peel")  one SUB-ROUND over the queue slice [lo, hi) fixed at launch: for every entry u != v of row v,
//                            if atomic load deg[u] > k:  old = fetch_sub(deg[u], 1)
//                               old == k + 1: append u at tail           (exactly once per vertex: see below)
//                               old <= k:     fetch_add(deg[u], 1) back  (somebody else took it to k first)
//   turn   (one thread)    lo = hi, hi = tail; an empty slice ends the level: k += 1, phase = scan; otherwise phase = peel;
//                          tail == n: done (everything still queued has only queued neighbours)
// The transient dip below k is harmless: a vertex's word never rises above k again -- it is raised only by the restore that is
// paired with a dip -- so `old == k + 1` is seen once, and it never wraps: a vertex is decremented at most once per neighbour.
// The peel is the walk of gl_rows.h over the rows of the queued vertices, a thread per queued vertex; the wavefront takes over
// a row still unfinished after kcore_cut = 8 entries (late levels consist of hub rows).  A slice shorter than the launch has
// wavefronts gives every wavefront fewer vertices.
// MEMORY RULE and GATING: gl_rounds.h.  Atomic-only inside a peel launch: deg[] and the tail (the queue slice and the control
// record were written by earlier launches; queue words written now are read by later ones).  The host enqueues (scan, peel,
// turn) x kcore_batch, of which exactly one of scan / peel runs per triple -- a scan that finds the phase "peel" returns at once
// and vice versa.  At most n sub-rounds and n + 1 levels exist, so the loop is capped.
// The control record is gl_rounds.h's peel record (kPeelLevel = k, kPeelTop = the degeneracy); the tail is the only word of it that a
// scan or peel launch writes.
#include "gl_rounds.h"

namespace gl {

// deg[v] = entries of row v other than v itself (the rows are sets of columns < n), the control record of level 0
__global__ __launch_bounds__(256) void kcore_init_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                         uint32_t n, uint32_t nz_base, uint32_t *__restrict__ deg, uint32_t *__restrict__ ctl) {
    if (blockIdx.x == 0u && threadIdx.x < 64u) ctl[threadIdx.x] = 0u;      // k = 0, an empty slice at 0, phase scan, tail 0
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t b = row_ptr[v] - nz_base, len = row_ptr[v + 1u] - nz_base - b;
        uint32_t d = len;
        if (len != 0u && row_idx[b + rows_lower_bound(row_idx + b, len, (uint32_t)v)] == (uint32_t)v) d -= 1u;
        deg[v] = d;
    }
}

__global__ __launch_bounds__(256) void kcore_scan_kernel(const uint32_t *__restrict__ deg, uint32_t *__restrict__ queue, uint32_t *ctl,
                                                         uint32_t n) {
    if (ctl[kPeelPhase] != kPeelScan) return;
    const uint32_t k = ctl[kPeelLevel], lane = threadIdx.x & 63u;
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;       // whole wavefronts take every trip
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += gridDim.x * 256u) {
        const bool hit = v < n && deg[v] == k;
        const uint32_t pos = wave_append(hit, ctl + kPeelTail, lane);
        if (hit && pos < n) queue[pos] = (uint32_t)v;             // (pos < n: every vertex is appended once)
    }
}

struct KcPeelArgs {
    const uint32_t *row_ptr, *row_idx;
    uint32_t *deg, *queue, *ctl;
    uint32_t n, nz_base, cut_steps;
};

// one neighbour u of a vertex peeled at level k
__device__ __forceinline__ void kc_relax(const KcPeelArgs &a, uint32_t u, uint32_t k) {
    if (ga_load(a.deg + u) <= k) return;                          // peeled before, or queued at this level
    const uint32_t old = ga_sub(a.deg + u, 1u);
    if (old == k + 1u) {
        const uint32_t pos = ga_add(a.ctl + kPeelTail, 1u);
        if (pos < a.n) a.queue[pos] = u;
    } else if (old <= k) {
        (void)ga_add(a.deg + u, 1u);
    }
}

__global__ __launch_bounds__(256) void kcore_peel_kernel(KcPeelArgs a) {
    if (a.ctl[kPeelPhase] != kPeelPeel) return;
    const uint32_t k = a.ctl[kPeelLevel], lo = a.ctl[kPeelLo], hi = a.ctl[kPeelHi];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t count = hi - lo, nwaves = gridDim.x * 4u;
    // queued vertices per wavefront: 64, fewer when the slice is shorter than the launch (late levels: a few hub rows) -- a
    // guess that was not measured against the plain 64 per wavefront
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    const uint32_t nwords = (uint32_t)(((uint64_t)count + per - 1u) / per);
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t item = (uint64_t)wd * per + lane;
        const bool in = lane < per && item < count;
        uint32_t v = 0, beg = 0, end = 0;
        if (in) {
            v = a.queue[lo + item];
            beg = a.row_ptr[v] - a.nz_base;
            end = a.row_ptr[v + 1u] - a.nz_base;
        }
        rows_walk_thread(a.row_idx, beg, end, a.cut_steps, [&](const uint32_t(&c)[4], uint32_t) {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c[u] < a.n && c[u] != v) kc_relax(a, c[u], k);
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t row = __shfl(v, src);
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n && c[u] != row) kc_relax(a, c[u], k);
                return false;
            });
        });
    }
}

// behind exactly one scan or peel that ran (plain loads and stores: a launch of its own)
__global__ void kcore_turn_kernel(uint32_t *ctl, uint32_t n) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    const uint32_t phase = ctl[kPeelPhase];
    if (phase == kPeelDone) return;
    const uint32_t k = ctl[kPeelLevel], lo = ctl[kPeelHi], hi = ctl[kPeelTail];
    if (phase == kPeelPeel) ctl[kPeelSubRounds] += 1u;
    ctl[kPeelLo] = lo;
    ctl[kPeelHi] = hi;
    const bool done = hi >= n, over = lo == hi;
    if ((done || over) && hi != ctl[kPeelLevelStart]) {             // the level queued somebody: its vertices have core k
        ctl[kPeelLevels] += 1u;
        ctl[kPeelLevelStart] = hi;
        ctl[kPeelTop] = k;
    }
    if (done) {
        ctl[kPeelPhase] = kPeelDone;
    } else if (over) {
        ctl[kPeelLevel] = k + 1u;
        ctl[kPeelPhase] = kPeelScan;
    } else {
        ctl[kPeelPhase] = kPeelPeel;
    }
}

// the refusals, the plan's verdicts and its scratch, on first use
static int kcore_prepare(gl_spmv_plan p, const char *who) {
    const int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_simple");
    if (rc != GL_OK || p->nnz == 0) return rc;
    // the control record, then the queue of a call without d_order
    return plan_scratch(p->d_kcore_scratch, kRoundsCtlBytes + 4u * (size_t)p->num_rows, who, "control record and queue");
}

static int kcore(gl_spmv_plan p, uint32_t *d_core, uint32_t *d_order, uint32_t *h_stats, const char *who) {
    int rc = kcore_prepare(p, who);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_rows;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0u;
    if (n == 0u) return GL_OK;
    if (p->nnz == 0) {                                            // an empty graph: nobody has a neighbour, any order will do
        GL_HIP(hipMemsetAsync(d_core, 0, 4u * (size_t)n, s));
        return d_order ? rows_iota(d_order, n) : GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call): kcore_cut = entries a thread reads before the wavefront takes the row over,
    // kcore_batch = (scan, peel, turn) triples enqueued between two read-backs of the control record (8 and 64: the best of
    // 8 / 32 / 128 and of 1 / 4 / 16 / 64, EXPERIMENTS.md Round 13), kcore_grid = workgroups per compute unit of a peel launch
    // (4: an unmeasured guess, no A/B was run)
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("kcore_cut", 8), 1l << 30, debug_knob("kcore_grid", 4));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("kcore_batch", 64), 4096));
    uint32_t *ctl = reinterpret_cast<uint32_t *>(p->d_kcore_scratch);
    KcPeelArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.deg = d_core;
    a.queue = d_order ? d_order : ctl + kRoundsCtlBytes / 4u;
    a.ctl = ctl;
    a.n = n;
    a.nz_base = p->csr_nz_base;
    a.cut_steps = shape.cut_steps;
    const unsigned stream_grid = rows_stream_grid(n), peel_grid = shape.grid;
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    static_assert(kPeelRecordWords * 4u <= 64u, "the record fits the page-locked staging words");
    kcore_init_kernel<<<stream_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, n, a.nz_base, d_core, ctl);
    GL_LAUNCH_CHECK();
    uint64_t launches = 1;
    // every step that runs is a scan (one per level, and k never passes the degeneracy < n) or a sub-round over a slice that is
    // not empty (every vertex is in one slice): at most 2 n + 1 steps
    rc = rounds_run(
        batch, 2ull * n + 1ull, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                kcore_scan_kernel<<<stream_grid, 256, 0, s>>>(d_core, a.queue, ctl, n);
                kcore_peel_kernel<<<peel_grid, 256, 0, s>>>(a);
                kcore_turn_kernel<<<1, 64, 0, s>>>(ctl, n);
            }
            return 3ull * batch;
        },
        [&] { return hipMemcpyAsync(w, ctl, kPeelRecordWords * 4u, hipMemcpyDeviceToHost, s); },
        [&] { return w[kPeelPhase] == kPeelDone ? kRoundsDone : kRoundsGoOn; },
        [&](uint64_t steps) {
            return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu steps on %u vertices (level %u, %u sub-rounds)", who,
                             (unsigned long long)steps, n, w[kPeelLevel], w[kPeelSubRounds]);
        });
    if (rc != GL_OK) return rc;
    if (h_stats) {
        h_stats[0] = w[kPeelTop];
        h_stats[1] = w[kPeelLevels];
        h_stats[2] = w[kPeelSubRounds];
        h_stats[3] = (uint32_t)std::min<uint64_t>(launches, 0xffffffffull);
    }
    return GL_OK;
}

}  // namespace gl

int gl_kcore(gl_spmv_plan plan, uint32_t *d_core, uint32_t *d_order, uint32_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_core != nullptr);
    GL_ARG(d_order != d_core);
    return gl::kcore(plan, d_core, d_order, h_stats, "gl_kcore");
}
