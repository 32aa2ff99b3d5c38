// Minimum spanning forest (gl_msf): Boruvka's algorithm over the plain CSR copy that every GL_PLAN_BOOLEAN plan keeps
// (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base), on a square, whole-matrix plan whose rows are strictly ascending
// sets N(v) of columns below num_cols and whose pattern is SYMMETRIC, with one f32 WEIGHT word per entry handed in by the caller.
// An ENTRY is a stored (v, u); entry j is word j of the row copy.  An EDGE is the pair of entries (lo, hi), (hi, lo), lo < hi; its
// weight is the word of the entry ABOVE the diagonal, (lo, hi) -- the mirror entry's word is never read.
//
//   key(w)      = b ^ (b >> 31 ? 0xffffffff : 0x80000000), b the bits of w: the monotone map of f32 to uint32
//   edges are ordered by (key(w), lo, hi); ascending entry number j of (lo, hi) IS ascending (lo, hi), so the 64-bit word
//   key(w) << 32 | j realises the order and names the edge.  The order is strict and total, so the minimum spanning forest under
//   it is unique -- the one Kruskal's algorithm returns when it takes the edges in this order -- whatever the schedule.
//
// STATE, over n = num_cols vertices: comp[n] in two copies A and B (between rounds A == B and comp[v] is the ROOT of
// v's component, an arbitrary vertex of it), best[n] 64-bit words (the smallest edge word leaving the component of root c, all
// ones: none), first[n] (the first entry above the diagonal of every row, found once per call), a LIST of the forest edges
// {entry, smaller end} and a CONTROL RECORD {done, rounds, forest edges, ...} + one "changed" word per pointer-doubling step.
// ONE ROUND:
//   scan    (the hot path) streams the entries above the diagonal with the walk of gl_rows.h, the wavefront taking over a row
//           longer than `cut` such entries; a weight word is loaded beside every column.
//           An entry whose ends lie in different components is a candidate for both.  The row's own side is
//           reduced in registers (across the wavefront by shuffles for a taken-over row): one atomic min per row; the far side
//           costs one atomic min per candidate, filtered by a relaxed atomic load of the word it would lower (msf_offer: a thread
//           also remembers an upper bound of the word it last offered to, and skips what is not below it without a load).
//   hook    a thread per vertex copies A to B; a root c with a chosen edge e, whose other end lies in the component of root d,
//           writes B[c] = d, marks the entry and appends it to the list -- unless d chose the same edge and c < d: of such a pair
//           the smaller root stays root and the larger one records the edge, so an edge is recorded once.  Under a strict total
//           order these pairs are the only cycles among the choices (along a longer cycle the chosen words would have to descend
//           strictly all the way round).  The edge's smaller end is the row of its entry, found by binary search in row_ptr.
//   turn    (one wavefront) a round that hooked nothing sets done; otherwise rounds += 1; clears the "changed" words.
//   flatten pointer doubling B -> A -> B ... with one "changed" word per step; a step whose predecessor changed nothing returns at
//           once, and then A == B element for element.  ceil(log2 n) + 1 steps are enqueued: ONE round can hang n components into
//           a single chain (weights ascending along a path), so a walk to the root per vertex will not do.  The first step also
//           clears best[].
// AFTER done: the mirror entry (hi, lo) of every listed edge is found by rows_lower_bound in row hi and marked; with d_labels, every
// vertex lowers its root's word of B to itself (an atomic min) and the labels are gathered through A; the roots are counted.
// MEMORY RULE and GATING: gl_rounds.h.  What is atomic-only in which launch:
//   * inside the scan launch best[] (a relaxed atomic load, an atomic min); comp[], first[], the rows and the weights are read-only
//     in it (plain loads of words written by earlier launches);
//   * a word of best[] only descends within a launch, so the filter's load, however stale, can cost a needless atomic and never a
//     wrong skip: it skips only what is not below a value the word held at some time, hence not below its final value;
//   * the hook reads A and best[] plainly (written by earlier launches) and writes B, the marks and the list; no word it writes is
//     read in the same launch.  The list's tail is an agent-scope atomic add, one per wavefront;
//   * the "changed" word of a pointer-doubling step is touched only by agent-scope atomics (a load, an OR: once per workgroup) in
//     the launch that raises it, and read plainly by the next;
//   * the label pass lowers B[root] by agent-scope atomic mins only and reads A plainly; the gather runs behind a launch boundary.
// Every launch returns at once when the record says done, the closing passes unless it does: the host enqueues msf_batch rounds
// and the closing passes behind them.  A round that hooks at least halves the components that still have an edge, so at most
// ceil(log2 n) rounds hook and one more finds nothing.
// The jump and count kernels are private copies of gl_cc.hip's (they are gated and the first jump clears best[]): gl_cc is untouched.
#include "gl_rounds.h"
#include "graphlily_hip_msf.h"

namespace gl {

// the control record (words); the "changed" words of the pointer-doubling steps start at kMsfChanged
enum : uint32_t { kMsfDone = 0, kMsfRounds = 1, kMsfEdges = 2, kMsfSeen = 3, kMsfCount = 4, kMsfRecordWords = 5, kMsfChanged = 16 };
constexpr uint32_t kMsfMaxJumps = 36;      // ceil(log2 2^32) + 1, with room
constexpr unsigned long long kMsfNone = ~0ull;

__device__ __forceinline__ unsigned long long msf_word(uint32_t bits, uint32_t j) {
    const uint32_t key = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
    return ((unsigned long long)key << 32) | j;
}

// best[c] = min(best[c], word).  With the filter, only when a load finds the word above it.  {hc, hv} remember the component the
// thread last offered to and a value its word has held since: the word only descends, so hv bounds it from above, and a candidate
// that is not below hv is skipped WITHOUT a load -- a run of candidates for one component (late rounds: the giant one) costs few
// loads.  A candidate that is below hv is checked against a fresh load before it costs an atomic: thousands of atomics on one
// word cost far more than as many loads of it (EXPERIMENTS.md Round 19)
__device__ __forceinline__ void msf_offer(unsigned long long *best, uint32_t c, unsigned long long word, uint32_t filter, uint32_t &hc,
                                          unsigned long long &hv) {
    if (filter) {
        if (c == hc && hv <= word) return;
        hc = c;
        hv = ga_load(best + c);
        if (hv <= word) return;
        hv = word;
    }
    ga_min(best + c, word);
}

__device__ __forceinline__ unsigned long long msf_shfl_xor(unsigned long long x, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}

struct MsfArgs {
    const uint32_t *row_ptr, *row_idx, *weight;    // weight: the caller's f32 words, read as bits
    const uint32_t *first, *comp, *ctl;
    unsigned long long *best;
    uint32_t n, nz_base, cut_steps, filter;
};

// A[v] = B[v] = v, best[v] = none, first[v] = the first entry of row v above the diagonal (the row's end if there is none)
__global__ __launch_bounds__(256) void msf_begin_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                        uint32_t n, uint32_t nz_base, uint32_t *__restrict__ A, uint32_t *__restrict__ B,
                                                        unsigned long long *__restrict__ best, uint32_t *__restrict__ first) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t b = row_ptr[v] - nz_base, len = row_ptr[v + 1u] - nz_base - b;
        uint32_t at = len;
        if (len != 0u) {
            at = rows_lower_bound(row_idx + b, len, (uint32_t)v + 1u);       // (v + 1 <= n: no wrap; at < len)
            if (row_idx[b + at] <= (uint32_t)v) at = len;
        }
        A[v] = B[v] = (uint32_t)v;
        best[v] = kMsfNone;
        first[v] = b + at;
    }
}

__global__ __launch_bounds__(256) void msf_scan_kernel(MsfArgs a) {
    if (a.ctl[kMsfDone] != 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwords = (a.n + 63u) >> 6;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += gridDim.x * 4u) {
        const uint32_t row = wd * 64u + lane;
        uint32_t beg = 0, end = 0, cv = 0;
        if (row < a.n) {
            beg = a.first[row];
            end = a.row_ptr[row + 1u] - a.nz_base;
            cv = a.comp[row];
        }
        unsigned long long mine = kMsfNone;               // the smallest candidate of this row
        uint32_t hc = 0xffffffffu;                        // (no component: vertices are below n <= 2^32 - 1)
        unsigned long long hv = 0;
        // the weight words first: nothing sits between them and the index loads, so a step's loads are in flight together
        rows_walk_thread(a.row_idx, beg, end, a.cut_steps, [&](const uint32_t(&c)[4], uint32_t at) {
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = end - at > (uint32_t)u ? a.weight[at + u] : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (c[u] >= a.n) continue;
                const uint32_t cu = a.comp[c[u]];
                if (cu == cv) continue;
                const unsigned long long word = msf_word(w[u], at + u);
                mine = min(mine, word);
                msf_offer(a.best, cu, word, a.filter, hc, hv);
            }
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t cr = __shfl(cv, src);
            unsigned long long low = kMsfNone;
            if ((int)lane == src) {                       // (what its own thread found joins the wavefront's minimum)
                low = mine;
                mine = kMsfNone;
            }
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
                uint32_t w[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint64_t j = base + 64u * u + lane;
                    w[u] = j < e ? a.weight[j] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (c[u] >= a.n) continue;
                    const uint32_t cu = a.comp[c[u]];
                    if (cu == cr) continue;
                    const unsigned long long word = msf_word(w[u], (uint32_t)base + 64u * u + lane);   // (an entry: below 2^32)
                    low = min(low, word);
                    msf_offer(a.best, cu, word, a.filter, hc, hv);
                }
                return false;
            });
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) low = min(low, msf_shfl_xor(low, d));
            if (lane == 0u && low != kMsfNone) msf_offer(a.best, cr, low, a.filter, hc, hv);
        });
        if (mine != kMsfNone) msf_offer(a.best, cv, mine, a.filter, hc, hv);
    }
}

// B = A, except that a root with a chosen edge goes under the root at the edge's other end
__global__ __launch_bounds__(256) void msf_hook_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx, uint32_t n,
                                                       uint32_t nz_base, const uint32_t *__restrict__ A, uint32_t *__restrict__ B,
                                                       const unsigned long long *__restrict__ best, uint32_t *__restrict__ in_forest,
                                                       uint32_t *__restrict__ list, uint32_t *ctl) {
    if (ctl[kMsfDone] != 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;           // whole wavefronts take every trip
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < nround; i += gridDim.x * 256u) {
        const uint32_t c = (uint32_t)i;
        bool hooks = false;
        uint32_t j = 0, lo = 0;
        if (i < n) {
            uint32_t to = A[c];
            const unsigned long long e = to == c ? best[c] : kMsfNone;
            if (e != kMsfNone) {
                j = (uint32_t)e;
                uint32_t at = 0, len = n + 1u;                        // the last v with row_ptr[v] - nz_base <= j: j's row
                while (len > 1u) {
                    const uint32_t half = len >> 1;
                    at += row_ptr[at + half] - nz_base <= j ? half : 0u;
                    len -= half;
                }
                lo = at;
                const uint32_t ca = A[lo], cb = A[row_idx[j]];
                const uint32_t d = ca == c ? cb : ca;
                hooks = !(best[d] == e && c < d);                     // (of two roots that chose one edge the smaller stays root)
                if (hooks) to = d;
            }
            B[c] = to;
        }
        const uint32_t at = wave_append(hooks, ctl + kMsfEdges, lane);
        if (hooks && at < n) {                                        // (at < n: a forest has fewer edges than vertices)
            in_forest[j] = 1u;
            list[2u * at] = j;
            list[2u * at + 1u] = lo;
        }
    }
}

// behind a hook (plain loads and stores: a launch of its own)
__global__ void msf_turn_kernel(uint32_t *ctl, uint32_t jumps) {
    if (blockIdx.x != 0u || ctl[kMsfDone] != 0u) return;
    if (threadIdx.x < jumps) ctl[kMsfChanged + threadIdx.x] = 0u;
    if (threadIdx.x != 0u) return;
    const uint32_t edges = ctl[kMsfEdges];
    if (edges == ctl[kMsfSeen]) ctl[kMsfDone] = 1u;
    else ctl[kMsfRounds] += 1u;
    ctl[kMsfSeen] = edges;
}

// one step of pointer doubling: out[v] = in[in[v]]; changed[step] != 0 if some vertex moved.  A step whose predecessor changed
// nothing returns at once: in == out already, element for element.  The first step of a round clears best[].
__global__ __launch_bounds__(256) void msf_jump_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t n, uint32_t *ctl,
                                                       uint32_t step, unsigned long long *__restrict__ best) {
    if (ctl[kMsfDone] != 0u) return;
    if (step != 0u && ctl[kMsfChanged + step - 1u] == 0u) return;
    bool moved = false;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t p = in[v], g = in[p];
        out[v] = g;
        moved |= g != p;
        if (best) best[v] = kMsfNone;
    }
    // one word for the whole launch, raised once per workgroup and only if a load finds it down: thousands of atomics on one
    // address were most of a step's time (EXPERIMENTS.md Round 19).  The word only rises, so a stale load costs a needless atomic
    if (__syncthreads_or(moved) && threadIdx.x == 0u && ga_load(ctl + kMsfChanged + step) == 0u) atomicOr(ctl + kMsfChanged + step, 1u);
}

// the closing passes: each runs once, in the batch whose turn said done
__global__ __launch_bounds__(256) void msf_mirror_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx, uint32_t n,
                                                         uint32_t nz_base, const uint32_t *__restrict__ list, uint32_t *__restrict__ in_forest,
                                                         const uint32_t *ctl) {
    if (ctl[kMsfDone] == 0u) return;
    const uint32_t edges = min(ctl[kMsfEdges], n);
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < edges; i += gridDim.x * 256u) {
        const uint32_t j = list[2u * i], lo = list[2u * i + 1u], hi = row_idx[j];
        const uint32_t b = row_ptr[hi] - nz_base, len = row_ptr[hi + 1u] - nz_base - b;    // (len >= 1: the pattern is symmetric)
        const uint32_t at = rows_lower_bound(row_idx + b, len, lo);
        if (row_idx[b + at] == lo) in_forest[b + at] = 1u;
    }
}

__global__ __launch_bounds__(256) void msf_label_min_kernel(const uint32_t *__restrict__ A, uint32_t *B, uint32_t n, const uint32_t *ctl) {
    if (ctl[kMsfDone] == 0u) return;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t r = A[v];
        if ((uint32_t)v < r) ga_min(B + r, (uint32_t)v);
    }
}

// labels[v] = B[A[v]] (with labels), and the roots are counted: one ballot per trip and one atomic add per wavefront
__global__ __launch_bounds__(256) void msf_finish_kernel(const uint32_t *__restrict__ A, const uint32_t *__restrict__ B, uint32_t n,
                                                         uint32_t *__restrict__ labels, uint32_t *ctl) {
    if (ctl[kMsfDone] == 0u) return;
    uint32_t roots = 0;   // per wavefront
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += gridDim.x * 256u) {
        uint32_t r = 0xffffffffu;
        if (v < n) {
            r = A[v];
            if (labels) labels[v] = B[r];
        }
        roots += (uint32_t)__popcll(__ballot(v < n && r == (uint32_t)v));
    }
    if ((threadIdx.x & 63u) == 0u && roots != 0u) atomicAdd(ctl + kMsfCount, roots);
}

// the words of the plan's scratch: the control record, best[n] (64-bit), then A, B and first of n words each and the list of 2 n
struct MsfLayout {
    uint32_t *ctl, *A, *B, *first, *list;
    unsigned long long *best;
    size_t bytes;
};
static MsfLayout msf_layout(gl_spmv_plan p) {
    const size_t n = std::max<size_t>(p->num_cols, 1u);
    MsfLayout t;
    t.ctl = reinterpret_cast<uint32_t *>(p->d_msf_scratch);
    t.best = reinterpret_cast<unsigned long long *>(p->d_msf_scratch + kRoundsCtlBytes);
    t.A = reinterpret_cast<uint32_t *>(t.best + n);
    t.B = t.A + n;
    t.first = t.B + n;
    t.list = t.first + n;
    t.bytes = kRoundsCtlBytes + 28u * n;
    return t;
}

static int msf(gl_spmv_plan p, const float *d_weight, uint32_t *d_in_forest, uint32_t *d_labels, uint64_t *h_stats, const char *who) {
    int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_weighted");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_cols;
    const unsigned vertex_grid = rows_stream_grid(n);
    // the launches that end in an atomic on ONE word per wavefront or workgroup (the jumps, the count) take fewer workgroups
    const unsigned word_grid = std::min<unsigned>(vertex_grid, (unsigned)ctx().num_cus * 2u);
    if (n == 0u || p->nnz == 0) {                                 // no entries: no forest words, every vertex its own component
        if (d_labels && n && (rc = rows_iota(d_labels, n)) != GL_OK) return rc;
        GL_HIP(hipStreamSynchronize(s));
        if (h_stats) {
            h_stats[0] = 0;
            h_stats[1] = n;
            h_stats[2] = 0;
            h_stats[3] = d_labels && n ? 1 : 0;
        }
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 19): msf_cut = entries above the diagonal a thread reads before
    // the wavefront takes the row over, msf_grid = workgroups per compute unit of a scan launch, msf_batch = rounds enqueued between
    // two read-backs of the control record, msf_filter = 0 sends every candidate's atomic min without the load in front of it
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("msf_cut", 32), 1l << 30, debug_knob("msf_grid", 64));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("msf_batch", 4), 64));
    rc = plan_scratch(p->d_msf_scratch, msf_layout(p).bytes, who, "control record, best edges, two component arrays, row starts and edge list");
    if (rc != GL_OK) return rc;
    const MsfLayout t = msf_layout(p);
    const uint64_t nnz = p->nnz;
    MsfArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.weight = reinterpret_cast<const uint32_t *>(d_weight);
    a.first = t.first;
    a.comp = t.A;
    a.ctl = t.ctl;
    a.best = t.best;
    a.n = n;
    a.nz_base = p->csr_nz_base;
    a.cut_steps = shape.cut_steps;
    a.filter = debug_knob("msf_filter", 1) != 0 ? 1u : 0u;
    const unsigned scan_grid = shape.grid;
    uint32_t jumps = 1;                                           // ceil(log2 n) + 1
    while ((1ull << (jumps - 1u)) < n) jumps++;
    static_assert(kMsfChanged * 4u + kMsfMaxJumps * 4u <= kRoundsCtlBytes && kMsfMaxJumps >= 33u, "one word per step");
    static_assert(kMsfRecordWords <= 16u, "the record fits the page-locked staging words");
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    GL_HIP(hipMemsetAsync(t.ctl, 0, kRoundsCtlBytes, s));
    GL_HIP(hipMemsetAsync(d_in_forest, 0, 4u * (size_t)nnz, s));
    msf_begin_kernel<<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, n, a.nz_base, t.A, t.B, t.best, t.first);
    GL_LAUNCH_CHECK();
    uint64_t launches = 1;
    // every round that hooks at least halves the components that still have an edge: ceil(log2 n) such rounds and one that finds
    // nothing, jumps of them; a batch more for room
    rc = rounds_run(
        batch, (uint64_t)jumps + batch, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                msf_scan_kernel<<<scan_grid, 256, 0, s>>>(a);
                msf_hook_kernel<<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, n, a.nz_base, t.A, t.B, t.best, d_in_forest, t.list, t.ctl);
                msf_turn_kernel<<<1, 64, 0, s>>>(t.ctl, jumps);
                uint32_t *in = t.B, *out = t.A;
                for (uint32_t r = 0; r < jumps; r++) {
                    msf_jump_kernel<<<word_grid, 256, 0, s>>>(in, out, n, t.ctl, r, r == 0u ? t.best : nullptr);
                    std::swap(in, out);
                }
            }
            msf_mirror_kernel<<<vertex_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, n, a.nz_base, t.list, d_in_forest, t.ctl);
            if (d_labels) msf_label_min_kernel<<<vertex_grid, 256, 0, s>>>(t.A, t.B, n, t.ctl);
            msf_finish_kernel<<<word_grid, 256, 0, s>>>(t.A, t.B, n, d_labels, t.ctl);
            return (uint64_t)batch * (3u + jumps) + (d_labels ? 3u : 2u);
        },
        [&] { return hipMemcpyAsync(w, t.ctl, kMsfRecordWords * 4u, hipMemcpyDeviceToHost, s); },
        [&] { return w[kMsfDone] != 0u ? kRoundsDone : kRoundsGoOn; },
        [&](uint64_t rounds) {
            return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu rounds on %u vertices (%u rounds hooked, %u forest edges)", who,
                             (unsigned long long)rounds, n, w[kMsfRounds], w[kMsfEdges]);
        });
    if (rc != GL_OK) return rc;
    if ((uint64_t)w[kMsfEdges] + w[kMsfCount] != n)
        return set_error(GL_ERR_HIP, "%s: internal error: %u forest edges and %u components on %u vertices", who, w[kMsfEdges], w[kMsfCount], n);
    if (h_stats) {
        h_stats[0] = w[kMsfEdges];
        h_stats[1] = w[kMsfCount];
        h_stats[2] = w[kMsfRounds];
        h_stats[3] = launches;
    }
    return GL_OK;
}

}  // namespace gl

int gl_msf(gl_spmv_plan plan, const float *d_weight, uint32_t *d_in_forest, uint32_t *d_labels, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_weight != nullptr && d_in_forest != nullptr);
    GL_ARG(d_labels != d_in_forest);
    return gl::msf(plan, d_weight, d_in_forest, d_labels, h_stats, "gl_msf");
}
