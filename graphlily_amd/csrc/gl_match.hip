// Greedy weighted matching (gl_match): the locally dominant matching of Preis and of Manne and Bisseling over the plain
// CSR copy that every GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base), on a square,
// whole-matrix plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is SYMMETRIC, with one
// f32 WEIGHT word per entry handed in by the caller.  An ENTRY is a stored (v, u); entry j is word j of the row copy.  An EDGE is
// the pair of entries (lo, hi), (hi, lo), lo < hi; BOTH entries' words are read and must hold the same bits.
//
//   key(w)      = b ^ (b >> 31 ? 0xffffffff : 0x80000000), b the bits of w: gl_msf's monotone map of f32 to uint32
//   edges are ordered by (~key(w), lo, hi), ascending: heaviest first, among equal weights the smallest (lo, hi) first.  The order
//   is strict and total.  Seen from ONE end v the edges {v, u} are ordered by (~key(w), u): every u < v gives (u, v), every u > v
//   gives (v, u), and u < v < u' puts (u, v) before (v, u').  So the 64-bit word ~key(w) << 32 | u realises the order within a row.
// THE RESULT is the greedy matching in that order (take the edges one by one, keep an edge iff both ends are still free): unique,
// maximal, whatever the schedule.  It is computed as the locally dominant matching, which under a strict total order is the same
// set: an edge that is the best free edge of BOTH its ends is in the greedy matching of what is left, by induction over the order.
//
// STATE, over n = num_cols vertices: mate[n] (the caller's d_mate; 0xffffffff: free), cand[n] (the vertex v points
// to, 0xffffffff: none), two LISTS of n words each (this round's and the next round's vertices that must point), a FRESH list of n
// words (the vertices matched in this round) and a CONTROL RECORD.
// ONE ROUND, over the list of the vertices that must point (round 1: every vertex with a non-empty row):
//   point   (the hot path) every listed v reduces its row to the smallest word over the entries (v, u) with u != v, u < n and
//           mate[u] free, with the walk of gl_rows.h: a thread per row, the wavefront taking over a row longer than `cut` entries;
//           a weight word is loaded beside every column.  The reduction is in registers (across the wavefront by shuffles for a
//           taken-over row).  v owns cand[v]: no atomics.  No free neighbour: cand[v] = none, and v is finished, unmatched.
//           A list that does not fill the launch is spread, fewer rows per wavefront and no thread steps (match_deal, below).
//   match   every listed v with u = cand[v] and cand[u] == v is matched to u -- whether or not u is in the list (u may have pointed
//           to v rounds ago).  mate[v] and mate[u] are claimed by compare-and-swap from free; the claim that succeeds puts that
//           vertex on the fresh list, so each end gets there once, whether one end or both are listed.
//   collect every fresh x walks its row; a free w with cand[w] == x must point again and is appended to the next list.  w has ONE
//           pointer, so it is found once; a pointer stays valid while its target is free (free neighbours only disappear), so
//           nobody else needs to rescan.  The fresh list is dealt as point's list is; a wavefront gathers its finds in LDS.
//   turn    (one thread) counts the round and its scans, makes the next list this one, clears the tails, and sets done when the
//           new list is empty.
// rounds = the rounds with a non-empty list, scans = the sum of the lists' lengths: properties of graph and weights.
// AFTER done: one streaming launch counts the pairs (v < mate[v]) and the STUCK vertices: free, pointing at a free vertex.  With the
// same bits in both entries of every edge there are none (the best free edge overall is the best of both its ends, so a round with
// free adjacent vertices matches a pair); with different bits the pointers can close a cycle (0 -> 1 -> 2 -> 0), nothing is matched,
// the next list is empty, and the call ends with GL_ERR_INVALID_ARG instead of a non-maximal result.
// MEMORY RULE and GATING: gl_rounds.h.  What is atomic-only in which launch:
//   * point reads mate[] and writes cand[v] of its own v plainly: mate[] was written by earlier launches, nobody reads cand[] here;
//   * match reads cand[] plainly (written by point, an earlier launch) and touches mate[] ONLY by agent-scope compare-and-swap;
//     the fresh list's tail is an agent-scope atomic add, one per wavefront;
//   * collect reads mate[], cand[], the fresh list and its tail plainly (earlier launches) and appends to the next list, tail by
//     agent-scope atomic add, one per wavefront and flush of the finds it holds in LDS; nobody reads that list in the same launch;
//   * turn is a launch of its own with plain loads and stores.
// Every launch returns at once when the record says done, the closing pass unless it does: the host enqueues match_batch rounds
// and the closing pass behind them.  Every round but the last matches at least one pair (or the next list is empty and the run is
// done), so at most floor(n / 2) + 1 rounds run.
#include "gl_rounds.h"
#include "graphlily_hip_match.h"

namespace gl {

// the control record (words): the first line is the turn's, the second is added to by the launches between two turns
enum : uint32_t { kMatchDone = 0, kMatchRounds = 1, kMatchScans = 2 /* and 3: 64 bits */, kMatchCount = 4, kMatchWhich = 5, kMatchRecordWords = 6,
                  kMatchFresh = 32, kMatchNext = 33, kMatchPairs = 34, kMatchStuck = 35 };
constexpr uint32_t kMatchFree = 0xffffffffu;      // mate[v]: free; cand[v]: none (vertices are below n <= 2^32 - 1)
constexpr unsigned long long kMatchNone = ~0ull;

__device__ __forceinline__ unsigned long long match_word(uint32_t bits, uint32_t u) {
    const uint32_t key = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
    return ((unsigned long long)~key << 32) | u;
}

__device__ __forceinline__ unsigned long long match_shfl_xor(unsigned long long x, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}

struct MatchArgs {
    const uint32_t *row_ptr, *row_idx, *weight;    // weight: the caller's f32 words, read as bits
    uint32_t *mate, *cand, *lists, *fresh, *ctl;   // lists: 2 n words, list `which` at lists + which * n
    uint32_t n, nz_base, cut_steps, spread;
};

// How a list of `count` rows is dealt to the wavefronts of a launch.  64 rows each, a thread per row up to the cut, while the list
// fills the launch.  A shorter list is SPREAD: fewer rows per wavefront -- a power of two, at most `spread`, down to one -- and these
// rows go to the whole wavefront at once (no thread steps).  The takeover serves a wavefront's long rows one after the other, each
// waiting for its loads and gathers, and up to 64 such waits in a row were most of a late round's time (EXPERIMENTS.md Round 22).
struct MatchDeal {
    uint32_t per_wave, words, cut_steps;
};
__device__ __forceinline__ MatchDeal match_deal(uint32_t count, uint32_t cut_steps, uint32_t spread) {
    const uint64_t waves = (uint64_t)gridDim.x * 4u;
    uint32_t per = 64;
    while (per > 1u && (uint64_t)count <= waves * (per >> 1)) per >>= 1;
    if (per > spread) per = 64;
    return {per, (uint32_t)(((uint64_t)count + per - 1u) / per), per == 64u ? cut_steps : 0u};
}

// mate[v] = free, cand[v] = none; the vertices with a non-empty row go to the next list, which the first turn makes round 1's
__global__ __launch_bounds__(256) void match_begin_kernel(MatchArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *next = a.lists + (size_t)(a.ctl[kMatchWhich] ^ 1u) * a.n;
    const uint64_t nround = ((uint64_t)a.n + 255u) & ~255ull;         // whole wavefronts take every trip
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += gridDim.x * 256u) {
        bool rows = false;
        if (v < a.n) {
            a.mate[v] = kMatchFree;
            a.cand[v] = kMatchFree;
            rows = a.row_ptr[v + 1u] != a.row_ptr[v];
        }
        const uint32_t at = wave_append(rows, a.ctl + kMatchNext, lane);
        if (rows && at < a.n) next[at] = (uint32_t)v;
    }
}

__global__ __launch_bounds__(256) void match_point_kernel(MatchArgs a) {
    if (a.ctl[kMatchDone] != 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t count = min(a.ctl[kMatchCount], a.n);
    const uint32_t *list = a.lists + (size_t)a.ctl[kMatchWhich] * a.n;
    const MatchDeal deal = match_deal(count, a.cut_steps, a.spread);
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < deal.words; wd += gridDim.x * 4u) {
        const uint32_t i = lane < deal.per_wave ? wd * deal.per_wave + lane : count;      // (below count + 64: no wrap)
        uint32_t v = 0, beg = 0, end = 0;
        if (i < count) {
            v = list[i];
            beg = a.row_ptr[v] - a.nz_base;
            end = a.row_ptr[v + 1u] - a.nz_base;
        }
        unsigned long long mine = kMatchNone;             // the smallest word of this row
        // the weight words first: nothing sits between them and the index loads, so a step's loads are in flight together
        rows_walk_thread(a.row_idx, beg, end, deal.cut_steps, [&](const uint32_t(&c)[4], uint32_t at) {
            uint32_t w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = end - at > (uint32_t)u ? a.weight[at + u] : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (c[u] < a.n && c[u] != v && a.mate[c[u]] == kMatchFree) mine = min(mine, match_word(w[u], c[u]));
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t vr = __shfl(v, src);
            unsigned long long low = kMatchNone;
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
                uint32_t w[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint64_t j = base + 64u * u + lane;
                    w[u] = j < e ? a.weight[j] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < a.n && c[u] != vr && a.mate[c[u]] == kMatchFree) low = min(low, match_word(w[u], c[u]));
                return false;
            });
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) low = min(low, match_shfl_xor(low, d));
            if ((int)lane == src) mine = min(mine, low);  // (what its own thread found before the cut stays in)
        });
        if (i < count) a.cand[v] = mine == kMatchNone ? kMatchFree : (uint32_t)mine;
    }
}

__global__ __launch_bounds__(256) void match_pair_kernel(MatchArgs a) {
    if (a.ctl[kMatchDone] != 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t count = min(a.ctl[kMatchCount], a.n);
    const uint32_t *list = a.lists + (size_t)a.ctl[kMatchWhich] * a.n;
    const uint64_t nround = ((uint64_t)count + 255u) & ~255ull;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < nround; i += gridDim.x * 256u) {
        uint32_t v = 0, u = kMatchFree;
        bool got_v = false, got_u = false;
        if (i < count) {
            v = list[i];
            u = a.cand[v];
            if (u != kMatchFree && a.cand[u] == v) {      // (u < n: point stores only columns below n)
                uint32_t expect = kMatchFree;
                got_v = ga_cas(a.mate + v, expect, u);
                expect = kMatchFree;
                got_u = ga_cas(a.mate + u, expect, v);
            }
        }
        uint32_t at = wave_append(got_v, a.ctl + kMatchFresh, lane);
        if (got_v && at < a.n) a.fresh[at] = v;           // (at < n: a vertex is matched once)
        at = wave_append(got_u, a.ctl + kMatchFresh, lane);
        if (got_u && at < a.n) a.fresh[at] = u;
    }
}

// The next list's tail is ONE word: an atomic add per wavefront and step on it was two thirds of a call's kernel time (EXPERIMENTS.md
// Round 22).  So every wavefront gathers its finds in kMatchHold words of LDS of its own -- positions from a ballot, the count in a
// register, no barrier: one wavefront's LDS accesses execute in order -- and moves them out with one atomic add per flush.
constexpr uint32_t kMatchHold = 512;

__global__ __launch_bounds__(256) void match_collect_kernel(MatchArgs a) {
    if (a.ctl[kMatchDone] != 0u) return;
    __shared__ uint32_t hold[4][kMatchHold];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t count = min(a.ctl[kMatchFresh], a.n);
    uint32_t *next = a.lists + (size_t)(a.ctl[kMatchWhich] ^ 1u) * a.n;
    uint32_t *q = hold[wave];
    const MatchDeal deal = match_deal(count, a.cut_steps, a.spread);
    uint32_t held = 0;                                    // the same in every lane
    auto flush = [&] {
        uint32_t base = 0;
        if (lane == 0u && held != 0u) base = ga_add(a.ctl + kMatchNext, held);
        base = __shfl(base, 0);
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < held; i += 64u)
            if (base + i < a.n) next[base + i] = q[i];    // (below n: a vertex has one pointer, so it is found once a round)
        __builtin_amdgcn_wave_barrier();
        held = 0;
    };
    // w points at x and is free: it must point again.  (The partner of x points at x too, and is not free.)  Both words are loaded
    // whatever the first says: the walk waits for its gathers, and two in flight cost no more than one
    auto find = [&](uint32_t w, uint32_t x) {             // called by every lane of the wavefront
        uint32_t cw = kMatchFree, mw = 0u;
        if (w < a.n) {
            cw = a.cand[w];
            mw = a.mate[w];
        }
        const bool h = w < a.n && cw == x && mw == kMatchFree;
        if (held > kMatchHold - 64u) flush();
        const unsigned long long m = __ballot(h);
        if (h) q[held + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = w;
        held += (uint32_t)__popcll(m);
    };
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < deal.words; wd += gridDim.x * 4u) {
        const uint32_t i = lane < deal.per_wave ? wd * deal.per_wave + lane : count;
        uint32_t x = kMatchFree, beg = 0, end = 0;
        if (i < count) {
            x = a.fresh[i];
            beg = a.row_ptr[x] - a.nz_base;
            end = a.row_ptr[x + 1u] - a.nz_base;
        }
        // rows_walk_thread's steps, with every lane of the wavefront in every step: the ballot wants them all
        for (uint32_t step = 0; step < deal.cut_steps && __any(beg < end); step++) {
            uint32_t c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) c[u] = beg < end && end - beg > (uint32_t)u ? a.row_idx[beg + u] : 0xffffffffu;
#pragma unroll
            for (int u = 0; u < 4; u++) find(c[u], x);
            beg += min(4u, end - beg);                    // (beg <= end: a finished row stays where it is)
        }
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t xr = __shfl(x, src);
            rows_walk_wave(a.row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
#pragma unroll
                for (int u = 0; u < 4; u++) find(c[u], xr);
                return false;
            });
        });
    }
    flush();
}

// behind a collect, and once behind the begin (plain loads and stores: a launch of its own)
__global__ void match_turn_kernel(uint32_t *ctl) {
    if (blockIdx.x != 0u || threadIdx.x != 0u || ctl[kMatchDone] != 0u) return;
    const uint32_t count = ctl[kMatchCount], next = ctl[kMatchNext];
    if (count != 0u) {
        ctl[kMatchRounds] += 1u;
        *reinterpret_cast<unsigned long long *>(ctl + kMatchScans) += count;
    }
    ctl[kMatchCount] = next;
    ctl[kMatchWhich] ^= 1u;
    ctl[kMatchFresh] = 0u;
    ctl[kMatchNext] = 0u;
    if (next == 0u) ctl[kMatchDone] = 1u;
}

// the closing pass: runs once, in the batch whose turn said done.  One ballot per trip and one atomic add per wavefront and word
__global__ __launch_bounds__(256) void match_finish_kernel(const uint32_t *__restrict__ mate, const uint32_t *__restrict__ cand, uint32_t n,
                                                           uint32_t *ctl) {
    if (ctl[kMatchDone] == 0u) return;
    uint32_t pairs = 0, stuck = 0;   // per wavefront
    const uint64_t nround = ((uint64_t)n + 255u) & ~255ull;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < nround; v += gridDim.x * 256u) {
        bool pair = false, bad = false;
        if (v < n) {
            const uint32_t m = mate[v], c = cand[v];
            pair = m != kMatchFree && (uint32_t)v < m;
            bad = m == kMatchFree && c != kMatchFree && mate[c] == kMatchFree;
        }
        pairs += (uint32_t)__popcll(__ballot(pair));
        stuck += (uint32_t)__popcll(__ballot(bad));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (pairs != 0u) atomicAdd(ctl + kMatchPairs, pairs);
        if (stuck != 0u) atomicAdd(ctl + kMatchStuck, stuck);
    }
}

__global__ __launch_bounds__(256) void match_free_kernel(uint32_t *__restrict__ mate, uint32_t n) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) mate[v] = kMatchFree;
}

// the words of the plan's scratch: the control record, then cand, the two lists and the fresh list of n words each
constexpr size_t match_scratch_bytes(size_t n) { return kRoundsCtlBytes + 16u * n; }

static int match(gl_spmv_plan p, const float *d_weight, uint32_t *d_mate, uint64_t *h_stats, const char *who) {
    int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_weighted");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_cols;
    const unsigned vertex_grid = rows_stream_grid(n);
    if (n == 0u || p->nnz == 0) {                                 // no entries: every vertex is free
        if (n) {
            match_free_kernel<<<vertex_grid, 256, 0, s>>>(d_mate, n);
            GL_LAUNCH_CHECK();
        }
        GL_HIP(hipStreamSynchronize(s));
        if (h_stats) {
            h_stats[0] = h_stats[1] = h_stats[2] = 0;
            h_stats[3] = n ? 1 : 0;
        }
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 22): match_cut = entries a thread reads before the wavefront
    // takes the row over, match_grid = workgroups per compute unit of a point or collect launch, match_batch = rounds enqueued
    // between two read-backs of the control record, match_spread = the most rows per wavefront a short list is spread to (0: never)
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("match_cut", 32), 1l << 30, debug_knob("match_grid", 64));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("match_batch", 8), 64));
    const size_t cells = std::max<size_t>(n, 1u);
    rc = plan_scratch(p->d_match_scratch, match_scratch_bytes(cells), who, "control record, pointers, two vertex lists and the fresh list");
    if (rc != GL_OK) return rc;
    MatchArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.weight = reinterpret_cast<const uint32_t *>(d_weight);
    a.mate = d_mate;
    a.ctl = reinterpret_cast<uint32_t *>(p->d_match_scratch);
    a.cand = reinterpret_cast<uint32_t *>(p->d_match_scratch + kRoundsCtlBytes);
    a.lists = a.cand + cells;
    a.fresh = a.lists + 2u * cells;
    a.n = n;
    a.nz_base = p->csr_nz_base;
    a.cut_steps = shape.cut_steps;
    a.spread = (uint32_t)std::max<long>(0, std::min<long>(debug_knob("match_spread", 16), 32));
    // a point or collect launch: the walk's grid, and never fewer wavefronts than would spread a short list (a wavefront per vertex
    // at most, eight workgroups per compute unit at most)
    const unsigned walk_grid = std::max(shape.grid, std::min<unsigned>((unsigned)ctx().num_cus * 8u, cdiv(n, 4u)));
    static_assert(kMatchRecordWords <= 8u && (kMatchStuck + 1u) * 4u <= kRoundsCtlBytes, "the record and the two counts fit the staging words");
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    GL_HIP(hipMemsetAsync(a.ctl, 0, kRoundsCtlBytes, s));
    match_begin_kernel<<<vertex_grid, 256, 0, s>>>(a);
    match_turn_kernel<<<1, 64, 0, s>>>(a.ctl);
    GL_LAUNCH_CHECK();
    uint64_t launches = 2;
    rc = rounds_run(
        batch, (uint64_t)n / 2u + 1u + batch, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                match_point_kernel<<<walk_grid, 256, 0, s>>>(a);
                match_pair_kernel<<<vertex_grid, 256, 0, s>>>(a);
                match_collect_kernel<<<walk_grid, 256, 0, s>>>(a);
                match_turn_kernel<<<1, 64, 0, s>>>(a.ctl);
            }
            match_finish_kernel<<<vertex_grid, 256, 0, s>>>(a.mate, a.cand, n, a.ctl);
            return (uint64_t)batch * 4u + 1u;
        },
        [&] {
            const hipError_t e = hipMemcpyAsync(w, a.ctl, kMatchRecordWords * 4u, hipMemcpyDeviceToHost, s);
            return e != hipSuccess ? e : hipMemcpyAsync(w + 8, a.ctl + kMatchPairs, 8u, hipMemcpyDeviceToHost, s);
        },
        [&] { return w[kMatchDone] != 0u ? kRoundsDone : kRoundsGoOn; },
        [&](uint64_t rounds) {
            return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu rounds on %u vertices (%u rounds counted, %u vertices listed)", who,
                             (unsigned long long)rounds, n, w[kMatchRounds], w[kMatchCount]);
        });
    if (rc != GL_OK) return rc;
    if (w[9] != 0u)
        return set_error(GL_ERR_INVALID_ARG,
                         "%s: %u free vertices still point at a free vertex after %u rounds: the two entries of an edge carry different weight "
                         "bits, so the pointers close a cycle and the matching would not be maximal (d_weight must hold the same word in "
                         "(v, u) and (u, v); io.symmetrize_weighted prepares it)", who, w[9], w[kMatchRounds]);
    if (h_stats) {
        h_stats[0] = w[8];
        h_stats[1] = w[kMatchRounds];
        h_stats[2] = (uint64_t)w[kMatchScans] | ((uint64_t)w[kMatchScans + 1u] << 32);
        h_stats[3] = launches;
    }
    return GL_OK;
}

}  // namespace gl

int gl_match(gl_spmv_plan plan, const float *d_weight, uint32_t *d_mate, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_weight != nullptr && d_mate != nullptr);
    return gl::match(plan, d_weight, d_mate, h_stats, "gl_match");
}
