// Graph colouring (gl_color): Jones-Plassmann colouring in its work-efficient form with dependency counters (Hasenplaugh, Kaler,
// Schardl & Leiserson) over the plain CSR copy that every GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr /
// d_csr_indices / csr_nz_base), on a square, whole-matrix plan whose rows are strictly ascending sets N(v) of columns below
// num_cols and whose pattern is SYMMETRIC, over n = num_rows vertices.  An entry (v, v) is ignored.
//
//   key(v)    = (prio[v], v); u GOES BEFORE v iff prio[u] > prio[v], or prio[u] == prio[v] and u < v (no prio: all 0)
//   colour[v] = the smallest non-negative integer that no neighbour going before v has: sequential first-fit greedy in that
//               order, a pure function of (graph, prio) whatever the schedule
//   round[v]  = 1 + max round[u] over the neighbours u going before v (1 without any): the launch that colours v
//
// STATE: ONE word per vertex, which IS d_color -- 0x80000000 | pending while v is uncoloured, pending = the
// neighbours going before v that are not coloured yet; the colour afterwards (at most the degree, so below 2^31); a QUEUE of n
// words, which every vertex enters exactly once, when its pending count reaches 0; and a CONTROL RECORD {lo, hi, rounds, widest,
// done} + tail and the running maximum colour (a line of their own: the only record words a colour launch writes).
//   init   counts, for every v, the entries u != v of row v that go before v (one gather of prio[u] per entry; without prio
//          one binary search for v in the row), writes the state word and appends every v whose count is 0: one ballot and one
//          atomic add to tail per wavefront
//   round  over the queue slice [lo, hi) fixed at launch: for every queued v ONE pass over row v, reading each neighbour's word
//            coloured:    it goes before v (those going after v wait for v); its colour enters a bit mask
//            uncoloured:  it goes after v (all going before v are coloured: v's count is 0): old = fetch_sub(word, 1);
//                         old == 0x80000001: append u at tail                          (exactly once per vertex)
//          then colour[v] = the first clear bit.  Two vertices of one slice are never adjacent (the later one would still count
//          the earlier), so the words a launch reads as coloured were written by earlier launches, and the words of later
//          vertices are only decremented and keep their top bit: the per-vertex steps may run in any order.
//   turn   (one thread)  lo = hi, hi = tail; a slice that is not empty is a round: rounds += 1, widest = max(widest, hi - lo);
//          an empty one ends the run: done (with tail < n that cannot happen; it is flagged and reported as an internal error)
// The round is the walk of gl_rows.h over the rows of the queued vertices, a thread per queued vertex; the wavefront takes over
// a row still unfinished after color_cut = 8 entries, and walks it once per window (below); a wavefront that holds ONE vertex
// (most rounds are that narrow) hands the row to all its lanes at once.  Every
// step issues its state loads together, then its decrements, then its appends, so that up to four of each are in flight per
// lane.  FREE COLOUR: a thread that finishes its row alone saw at most 64 entries, so a 64-bit mask decides (a row of d
// entries cannot force a colour above d).  The wavefront searches in WINDOWS of 256 colours, four 64-bit masks per lane OR-ed
// across the lanes once per pass: its first pass re-reads the entries the thread had done (colours only), decrements behind
// them, and collects window 0; a full window is followed by a pass that only reads colours, for the next 256.  The decrements
// are never repeated.  A hub of d entries whose colour is c costs 1 + c / 256 passes over its row.
// MEMORY RULE and GATING: gl_rounds.h.  Atomic-only inside a round launch: the state words, the tail and the running maximum
// (the queue slice and the record were written by earlier launches; queue words written now are read by later ones; prio is
// never written).  The host enqueues (round, turn) x color_batch; a launch that finds `done` returns at once.  Every round that
// runs colours a vertex, so at most n exist and the loop is capped at n + 1 steps.
#include "gl_rounds.h"
#include "graphlily_hip_ext.h"

namespace gl {

// the control record (words); tail and the running maximum sit in the second 128-byte line
enum : uint32_t { kColLo = 0, kColHi = 1, kColRounds = 2, kColWidest = 3, kColDone = 4, kColRecordWords = 8, kColTail = 32, kColMax = 33,
                  kColReadWords = 34 };
enum : uint32_t { kColRunning = 0, kColFinished = 1, kColStuck = 2 };
constexpr uint32_t kColWait = 0x80000000u;       // the top bit of an uncoloured vertex's word
constexpr uint32_t kColNobody = 0x7fffffffu;     // stands for the word of an entry that is no neighbour: a colour in no window
constexpr uint32_t kColInitCut = 32;             // entries of a row that init counts in one thread (a guess that was not measured)

// does u go before v?  (u != v)
__device__ __forceinline__ bool col_before(uint32_t pu, uint32_t u, uint32_t pv, uint32_t v) { return pu > pv || (pu == pv && u < v); }

// the state words and the first slice's members; the record was zeroed by a memset in front of this launch (tail is added to here)
__global__ __launch_bounds__(256) void color_init_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                         const uint32_t *__restrict__ prio, uint32_t n, uint32_t nz_base,
                                                         uint32_t *__restrict__ state, uint32_t *__restrict__ queue, uint32_t *ctl) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;       // whole wavefronts take every trip
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < nround; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        const bool in = v64 < n;
        uint32_t beg = 0, end = 0, count = 0, pv = 0;
        if (in) {
            beg = row_ptr[v] - nz_base;
            end = row_ptr[v + 1u] - nz_base;
        }
        if (prio == nullptr) {                                    // the entries below v: the rows ascend
            if (beg < end) {
                const uint32_t at = rows_lower_bound(row_idx + beg, end - beg, v);
                count = at + (row_idx[beg + at] < v ? 1u : 0u);
            }
            beg = end;
        } else if (in) {
            pv = prio[v];
            if (end - beg <= kColInitCut) {
                for (; beg < end; beg++) {
                    const uint32_t u = row_idx[beg];
                    if (u < n && u != v && col_before(prio[u], u, pv, v)) count += 1u;
                }
            }
        }
        // longer rows are counted by the whole wavefront, 64 entries per step (coalesced index loads)
        for (uint64_t pending = __ballot(beg < end); pending; pending &= pending - 1ull) {
            const int src = __ffsll((unsigned long long)pending) - 1;
            const uint32_t b = __shfl(beg, src), e = __shfl(end, src), row = __shfl(v, src), pr = __shfl(pv, src);
            uint32_t c = 0;
            for (uint64_t base = b; base < e; base += 64u) {
                const uint64_t j = base + lane;
                const uint32_t u = j < e ? row_idx[j] : 0xffffffffu;
                const bool hit = u < n && u != row && col_before(prio[u], u, pr, row);
                c += (uint32_t)__popcll(__ballot(hit));
            }
            if ((int)lane == src) count = c;
        }
        if (in) state[v] = kColWait | count;                      // (plain: nobody reads it in this launch)
        const bool hit = in && count == 0u;
        const uint32_t pos = wave_append(hit, ctl + kColTail, lane);
        if (hit && pos < n) queue[pos] = v;                       // (pos < n: every vertex is appended once)
    }
}

struct ColRoundArgs {
    const uint32_t *row_ptr, *row_idx;
    uint32_t *state, *queue, *ctl;
    uint32_t n, nz_base, cut_steps;
};

// u's last earlier neighbour has just been coloured (the decrement that returned 0x80000001): u joins the queue
__device__ __forceinline__ void col_append(const ColRoundArgs &a, uint32_t u) {
    const uint32_t pos = ga_add(a.ctl + kColTail, 1u);
    if (pos < a.n) a.queue[pos] = u;
}

__device__ __forceinline__ unsigned long long col_wave_or(unsigned long long x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x |= __shfl_xor(x, d);
    return x;
}

__global__ __launch_bounds__(256) void color_round_kernel(ColRoundArgs a) {
    if (a.ctl[kColDone] != kColRunning) return;
    const uint32_t lo = a.ctl[kColLo], hi = a.ctl[kColHi];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t count = hi - lo, nwaves = gridDim.x * 4u;
    // queued vertices per wavefront: 64, fewer when the slice is shorter than the launch (as kcore_peel_kernel: not measured
    // against the plain 64 per wavefront)
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    const uint32_t nwords = (uint32_t)(((uint64_t)count + per - 1u) / per);
    // a wavefront with ONE vertex gives its row to all lanes at once: lane 0 walking the first color_cut entries alone only
    // adds dependent round trips (most rounds are this narrow)
    const uint32_t thread_steps = per == 1u ? 0u : a.cut_steps;
    uint32_t top = 0;                                             // the largest colour this lane stored
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t item = (uint64_t)wd * per + lane;
        const bool in = lane < per && item < count;
        uint32_t v = 0, first = 0, beg = 0, end = 0;
        if (in) {
            v = a.queue[lo + item];
            first = beg = a.row_ptr[v] - a.nz_base;
            end = a.row_ptr[v + 1u] - a.nz_base;
        }
        unsigned long long used = 0ull;                           // colours 0 .. 63 of the neighbours seen so far
        rows_walk_thread(a.row_idx, beg, end, thread_steps, [&](const uint32_t(&c)[4], uint32_t) {
            uint32_t w[4], old[4];
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = (c[u] < a.n && c[u] != v) ? ga_load(a.state + c[u]) : kColNobody;
#pragma unroll
            for (int u = 0; u < 4; u++) old[u] = (w[u] & kColWait) ? ga_sub(a.state + c[u], 1u) : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (old[u] == (kColWait | 1u)) col_append(a, c[u]);
                if (w[u] < 64u) used |= 1ull << w[u];
            }
            return false;
        });
        // a row finished here has at most 4 cut_steps <= 64 entries, so its colour is at most 64: the mask decides
        if (in && beg >= end) {
            const uint32_t colour = ~used ? (uint32_t)__ffsll(~used) - 1u : 64u;
            ga_store(a.state + v, colour);
            top = max(top, colour);
        }
        // a row taken over is walked from its FIRST entry, once per window
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t f = __shfl(first, src), row = __shfl(v, src);
            // window `wbase`: the colours wbase .. wbase + 255; the first pass also does the decrements behind b
            for (uint32_t wbase = 0, release_from = b;; wbase += 256u, release_from = e) {
                unsigned long long m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;
                rows_walk_wave(a.row_idx, f, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
                    // the four words, then the four decrements, then the appends: each kind in flight together
                    uint32_t w[4], old[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) w[u] = (c[u] < a.n && c[u] != row) ? ga_load(a.state + c[u]) : kColNobody;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        old[u] = ((w[u] & kColWait) && base + 64u * u + lane >= release_from) ? ga_sub(a.state + c[u], 1u) : 0u;
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (old[u] == (kColWait | 1u)) col_append(a, c[u]);
                        const uint32_t k = w[u] - wbase;
                        if (!(w[u] & kColWait) && k < 256u) {
                            const unsigned long long bit = 1ull << (k & 63u);
                            m0 |= k < 64u ? bit : 0ull;
                            m1 |= (k >> 6) == 1u ? bit : 0ull;
                            m2 |= (k >> 6) == 2u ? bit : 0ull;
                            m3 |= (k >> 6) == 3u ? bit : 0ull;
                        }
                    }
                    return false;
                });
                m0 = col_wave_or(m0);
                m1 = col_wave_or(m1);
                m2 = col_wave_or(m2);
                m3 = col_wave_or(m3);
                uint32_t colour = 0xffffffffu;
                if (~m0) colour = wbase + (uint32_t)__ffsll(~m0) - 1u;
                else if (~m1) colour = wbase + 64u + (uint32_t)__ffsll(~m1) - 1u;
                else if (~m2) colour = wbase + 128u + (uint32_t)__ffsll(~m2) - 1u;
                else if (~m3) colour = wbase + 192u + (uint32_t)__ffsll(~m3) - 1u;
                if (colour != 0xffffffffu) {                      // (uniform: every lane holds the same masks)
                    if ((int)lane == src) {
                        ga_store(a.state + row, colour);
                        top = max(top, colour);
                    }
                    break;
                }
            }
        });
    }
    // one atomic max per wavefront that coloured somebody above 0
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) top = max(top, (uint32_t)__shfl_xor(top, d));
    if (lane == 0u && top != 0u) ga_max(a.ctl + kColMax, top);
}

// behind a round (or init): plain loads and stores, a launch of its own
__global__ void color_turn_kernel(uint32_t *ctl, uint32_t n) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    if (ctl[kColDone] != kColRunning) return;
    const uint32_t lo = ctl[kColHi], hi = min(ctl[kColTail], n);
    ctl[kColLo] = lo;
    ctl[kColHi] = hi;
    if (hi == lo) {
        ctl[kColDone] = hi >= n ? kColFinished : kColStuck;       // (stuck: somebody still waits and nobody will release it)
    } else {
        ctl[kColRounds] += 1u;
        ctl[kColWidest] = max(ctl[kColWidest], hi - lo);
    }
}

// the refusals, the plan's verdicts and its scratch, on first use
static int color_prepare(gl_spmv_plan p, const char *who) {
    const int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_simple");
    if (rc != GL_OK || p->nnz == 0) return rc;
    return plan_scratch(p->d_color_scratch, kRoundsCtlBytes + 4u * (size_t)p->num_rows, who, "control record and queue");
}

static int color(gl_spmv_plan p, const uint32_t *d_prio, uint32_t *d_color, uint64_t *h_stats, const char *who) {
    int rc = color_prepare(p, who);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_rows;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0u;
    if (n == 0u) return GL_OK;
    if (p->nnz == 0) {                                            // an empty graph: one round colours everybody 0
        GL_HIP(hipMemsetAsync(d_color, 0, 4u * (size_t)n, s));
        if (h_stats) {
            h_stats[0] = h_stats[1] = 1u;
            h_stats[3] = n;
        }
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 17): color_cut = entries a thread reads before the wavefront
    // takes the row over (at most 64: what its one mask can decide) -- 8: 0 / 4 / 8 are within 1 % of each other, 16 / 32 / 64
    // were 13 - 95 % slower; color_batch = (round, turn) pairs enqueued between two read-backs of the control record -- 64: the
    // best of 1 / 4 / 16 / 64 / 256 (256 equals it within 1 % and enqueues more idle launches); color_grid = workgroups per compute
    // unit of a round launch -- 4: 1 / 2 / 16 are within 1 %, most rounds do not fill one workgroup per unit
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("color_cut", 8), 64, debug_knob("color_grid", 4));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("color_batch", 64), 4096));
    uint32_t *ctl = reinterpret_cast<uint32_t *>(p->d_color_scratch);
    ColRoundArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.state = d_color;
    a.queue = ctl + kRoundsCtlBytes / 4u;
    a.ctl = ctl;
    a.n = n;
    a.nz_base = p->csr_nz_base;
    a.cut_steps = shape.cut_steps;
    const unsigned stream_grid = rows_stream_grid(n), round_grid = shape.grid;
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    static_assert((kColRecordWords + kColReadWords - kColTail) * 4u <= 64u, "the record fits the page-locked staging words");
    GL_HIP(hipMemsetAsync(ctl, 0, kRoundsCtlBytes, s));
    color_init_kernel<<<stream_grid, 256, 0, s>>>(a.row_ptr, a.row_idx, d_prio, n, a.nz_base, d_color, a.queue, ctl);
    color_turn_kernel<<<1, 64, 0, s>>>(ctl, n);
    GL_LAUNCH_CHECK();
    uint64_t launches = 2;
    rc = rounds_run(
        batch, (uint64_t)n + 1ull, launches,                      // every round that runs colours a vertex
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                color_round_kernel<<<round_grid, 256, 0, s>>>(a);
                color_turn_kernel<<<1, 64, 0, s>>>(ctl, n);
            }
            return 2ull * batch;
        },
        [&] {
            const hipError_t e = hipMemcpyAsync(w, ctl, kColRecordWords * 4u, hipMemcpyDeviceToHost, s);
            return e != hipSuccess ? e : hipMemcpyAsync(w + kColRecordWords, ctl + kColTail, (kColReadWords - kColTail) * 4u, hipMemcpyDeviceToHost, s);
        },
        [&] { return w[kColDone] == kColFinished ? kRoundsDone : w[kColDone] == kColStuck ? kRoundsStuck : kRoundsGoOn; },
        [&](uint64_t steps) {
            return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu steps on %u vertices (%u rounds, %u vertices queued)", who,
                             (unsigned long long)steps, n, w[kColRounds], w[kColRecordWords]);
        });
    if (rc != GL_OK) return rc;
    if (h_stats) {
        h_stats[0] = (uint64_t)w[kColRecordWords + 1u] + 1u;
        h_stats[1] = w[kColRounds];
        h_stats[2] = launches;
        h_stats[3] = w[kColWidest];
    }
    return GL_OK;
}

}  // namespace gl

int gl_color(gl_spmv_plan plan, const uint32_t *d_prio, uint32_t *d_color, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_color != nullptr);
    GL_ARG(d_prio != d_color);
    return gl::color(plan, d_prio, d_color, h_stats, "gl_color");
}
