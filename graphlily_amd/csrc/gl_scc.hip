// Strongly connected components (gl_scc): trimming, then colour-and-collect passes (the colouring algorithm of Orzan, with the
// trimming of McLendon et al.) over the plain CSR copies that two GL_PLAN_BOOLEAN plans keep (gl_spmv_plan.h:
// d_csr_indptr / d_csr_indices / csr_nz_base): plan_in, whose row v holds the PREDECESSORS of v, and plan_out, the transposed
// pattern, whose row v holds its SUCCESSORS (plan_out == plan_in: a symmetric pattern).  Both are square whole-matrix plans whose
// rows are strictly ascending sets of columns below num_cols, over n = num_rows vertices.  An entry (v, v) is ignored.
//
//   key(v)   = ~prio[v] << 32 | v, a 64-bit word (no prio: all 0): the SMALLER key is the BETTER one -- larger prio first, then
//              the smaller vertex, gl_color's order.  0xffffffffffffffff (kSccDead) is no vertex's key and the worst of all.
//   label[v] = the smallest vertex u such that v reaches u and u reaches v: unique, whatever prio and the schedule.
//
// STATE: colour[n], 64-bit words -- the key of the best vertex known to reach v while v is LIVE, kSccDead once v
// has been given to a component (so "is u live" and "what is u's colour" are ONE gather, and a minimum over a row skips the dead
// by itself); root[n], which IS d_label -- written once, when v dies: a vertex of v's component, the same for all of it; mark[n]
// -- the colour (a vertex) under which v was found to reach its root, 0xffffffff before any; minv[n] -- starts as v; two LISTS
// of n words, this pass's live vertices and the next pass's; and a CONTROL RECORD.
// ONE PASS, over the list of the vertices that were live when it began (pass 1: every vertex with entries in both its rows):
//   trim      a live v without a live predecessor or without a live successor is a component of its own: root[v] = v, colour[v]
//             = dead.  Both walks stop at the first live neighbour.  Rounds until one removes nobody.  Nobody left: done.
//   forward   (the hot path) colour[v] = the smallest of colour[v] and colour[u] over the predecessors u, four words per step in
//             registers, ONE store per row, and only if the word got smaller.  Rounds until one changes nothing.  Then colour[v]
//             is the best key among the live vertices that reach v, and the vertices with colour[v] == key(v) are the ROOTS.
//   backward  a live v that is no root and is not marked becomes marked when a successor w is its colour's root or is marked
//             under that colour (mark[w] == the vertex of colour[v]): the walk stops at the first such w.  Rounds until one
//             marks nobody.  A root r is the best vertex of its own component (a better one in it would reach r), all of that
//             component carries key(r) (r reaches it, and whatever reaches it reaches r), and what reaches r INSIDE the colour
//             class is exactly the component (r reaches all of its class).
//   collect   (one launch) roots and marked vertices get root[v] = their colour's vertex and die; the others get colour[v] =
//             key(v) again and are appended to the next list (wave_append; its order is irrelevant).
//   turn      (one thread, behind every launch above) owns the phase word: it reads and clears the count of changes the launch
//             added up, counts the round, and moves to the next phase when a round changed nothing.
// The three fixed points are least fixed points of monotone maps, so they do not depend on the order of the evaluations: labels,
// PASSES (passes that reached forward) and TRIMMED (vertices removed by trim) are functions of (graph, prio).  ROUNDS is not: a
// read may see a word written earlier in the same launch, which can only bring a fixed point sooner than synchronous sweeps.
// AFTER done: one streaming launch does ga_min(minv[root[v]], v) and counts the components (root[v] == v), a second one does
// label[v] = minv[root[v]], in place.
// MEMORY RULE and GATING: gl_rounds.h.  What is atomic-only in which launch:
//   * trim      colour[] (liveness: read of the neighbours, written for the own vertex) and the change count; root[] is stored
//               plainly (nobody reads it before the closing launches);
//   * forward   colour[] and the change count;
//   * backward  mark[] and the change count; colour[] was written by earlier launches and is read plainly;
//   * collect   the next list's tail (one atomic add per wavefront); colour[], mark[] and root[] are read and written plainly,
//               every word by the thread of its own vertex only; nobody reads the next list in this launch;
//   * closing   minv[] by atomic min and the component count by atomic add in the first launch, plain in the second;
//   * turn      a launch of its own with plain loads and stores.
// No spin-waits, no tickets: every wait is a launch boundary.  The host enqueues (round, turn) x scc_batch and the two closing
// launches behind them; the round launch does the work of whatever phase the record names, the closing launches return at once
// unless it says done, and every launch returns at once when it does.
// STEP CAP: every pass that reaches forward removes at least its best-keyed live vertex (a root), so there are at most n passes.
// A trim round that is not a pass's last removes a vertex: at most n + passes of them.  A forward or backward fixed point is
// reached within (live vertices + 1) rounds, because a value travels along a simple path; pass p has at most n - p + 1 live
// vertices.  With one collect per pass that is at most n^2 + 6 n + 8 steps -- reached by nothing but a chain of components numbered
// against the priorities -- and a run beyond it, or a batch that does not move the record, is an internal error.
// SCRATCH, per plan_in: 256 + 24 n bytes -- the control record, colour (8 n), mark, minv and the two lists (4 n each).
#include "gl_rounds.h"
#include "graphlily_hip_scc.h"

namespace gl {

// the control record (words): the first line is the turn's, the second is added to by the launches between two turns
enum : uint32_t { kSccPhase = 0, kSccWhich = 1, kSccCount = 2, kSccAlive = 3, kSccPasses = 4, kSccTrimmed = 5, kSccSteps = 6 /* and 7 */,
                  kSccRounds = 8 /* and 9 */, kSccRecordWords = 10, kSccChanged = 32, kSccNext = 33, kSccComponents = 34 };
enum : uint32_t { kSccBegin = 0, kSccTrim = 1, kSccForward = 2, kSccBackward = 3, kSccCollect = 4, kSccDone = 5 };
constexpr unsigned long long kSccDead = ~0ull;
constexpr uint32_t kSccNoMark = 0xffffffffu;

struct SccArgs {
    const uint32_t *in_ptr, *in_idx, *out_ptr, *out_idx, *prio;
    unsigned long long *colour;
    uint32_t *root, *mark, *minv, *lists, *ctl;        // lists: 2 n words, list `which` at lists + which * n
    uint32_t n, in_base, out_base, cut_steps;
};

__device__ __forceinline__ unsigned long long scc_key(const SccArgs &a, uint32_t v) {
    return ((unsigned long long)~(a.prio ? a.prio[v] : 0u) << 32) | v;
}

__device__ __forceinline__ unsigned long long scc_wave_min(unsigned long long x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x = min(x, (unsigned long long)__shfl_xor(x, d));
    return x;
}

// How a list of `count` vertices is dealt to the wavefronts of a launch (as color_round_kernel deals its slice): 64 per wavefront,
// fewer when the list is shorter than the launch; a wavefront with ONE vertex gives the row to all its lanes at once.
struct SccDeal {
    uint32_t per, words, steps;
};
__device__ __forceinline__ SccDeal scc_deal(uint32_t count, uint32_t cut_steps) {
    const uint32_t nwaves = gridDim.x * 4u;
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    return {per, (uint32_t)(((uint64_t)count + per - 1u) / per), per == 1u ? 0u : cut_steps};
}

// Does the row [beg, end) of this lane's vertex hold a column c with hit(c, v, x)?  The walk of gl_rows.h, 64 rows per wavefront,
// which stops at the first hit.  v and x are the row's own; a row taken over by the wavefront gets them from its owner's lane.
template <typename Hit>
__device__ __forceinline__ bool scc_row_any(const uint32_t *__restrict__ row_idx, uint32_t beg, uint32_t end, uint32_t steps, uint32_t lane,
                                            uint32_t v, uint32_t x, Hit &&hit) {
    bool found = false;
    rows_walk_thread(row_idx, beg, end, steps, [&](const uint32_t(&c)[4], uint32_t) {
        bool h[4];
#pragma unroll
        for (int u = 0; u < 4; u++) h[u] = hit(c[u], v, x);
        found = h[0] || h[1] || h[2] || h[3];
        return found;
    });
    rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
        const uint32_t vr = __shfl(v, src), xr = __shfl(x, src);
        bool any = false;
        rows_walk_wave(row_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
            bool h[4];
#pragma unroll
            for (int u = 0; u < 4; u++) h[u] = hit(c[u], vr, xr);
            any = __any(h[0] || h[1] || h[2] || h[3]);
            return any;
        });
        if ((int)lane == src) found = any;
    });
    return found;
}

// one atomic add per wavefront: `mine` = this lane's changes
__device__ __forceinline__ void scc_count(uint32_t *word, uint32_t mine, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) mine += (uint32_t)__shfl_xor(mine, d);
    if (lane == 0u && mine != 0u) ga_add(word, mine);
}

// Every vertex: mark none, minv its own number.  A vertex with an empty row in either plan is a component of its own at once
// (counted as trimmed, through the change count); the others are live, get their own key and go to the next list, which the
// first turn makes pass 1's.  Plain stores: nobody reads these words in this launch.
__global__ __launch_bounds__(256) void scc_begin_kernel(SccArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *next = a.lists + (size_t)(a.ctl[kSccWhich] ^ 1u) * a.n;
    uint32_t gone = 0;
    const uint64_t nround = ((uint64_t)a.n + 255u) & ~255ull;       // whole wavefronts take every trip
    for (uint64_t v64 = blockIdx.x * 256u + threadIdx.x; v64 < nround; v64 += gridDim.x * 256u) {
        const uint32_t v = (uint32_t)v64;
        bool live = false;
        if (v64 < a.n) {
            live = a.in_ptr[v + 1u] != a.in_ptr[v] && a.out_ptr[v + 1u] != a.out_ptr[v];
            a.mark[v] = kSccNoMark;
            a.minv[v] = v;
            a.colour[v] = live ? scc_key(a, v) : kSccDead;
            if (!live) {
                a.root[v] = v;
                gone += 1u;
            }
        }
        const uint32_t at = wave_append(live, a.ctl + kSccNext, lane);
        if (live && at < a.n) next[at] = v;
    }
    scc_count(a.ctl + kSccChanged, gone, lane);
}

__device__ __forceinline__ void scc_trim(const SccArgs &a, const uint32_t *list, uint32_t count, uint32_t lane, uint32_t wave) {
    const SccDeal deal = scc_deal(count, a.cut_steps);
    // a live neighbour other than the vertex itself
    auto live_at = [&](uint32_t c, uint32_t v, uint32_t) { return c < a.n && c != v && ga_load(a.colour + c) != kSccDead; };
    uint32_t gone = 0;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < deal.words; wd += gridDim.x * 4u) {
        const uint64_t i = (uint64_t)wd * deal.per + lane;
        uint32_t v = 0, beg = 0, end = 0;
        bool live = false;
        if (lane < deal.per && i < count) {
            v = list[i];
            live = ga_load(a.colour + v) != kSccDead;
        }
        if (live) {
            beg = a.in_ptr[v] - a.in_base;
            end = a.in_ptr[v + 1u] - a.in_base;
        }
        const bool has_in = scc_row_any(a.in_idx, beg, end, deal.steps, lane, v, 0u, live_at);
        beg = end = 0;
        if (has_in) {
            beg = a.out_ptr[v] - a.out_base;
            end = a.out_ptr[v + 1u] - a.out_base;
        }
        const bool has_out = scc_row_any(a.out_idx, beg, end, deal.steps, lane, v, 0u, live_at);
        if (live && !has_out) {                                   // (has_out implies has_in)
            ga_store(a.colour + v, kSccDead);
            a.root[v] = v;
            gone += 1u;
        }
    }
    scc_count(a.ctl + kSccChanged, gone, lane);
}

__device__ __forceinline__ void scc_forward(const SccArgs &a, const uint32_t *list, uint32_t count, uint32_t lane, uint32_t wave) {
    const SccDeal deal = scc_deal(count, a.cut_steps);
    uint32_t changed = 0;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < deal.words; wd += gridDim.x * 4u) {
        const uint64_t i = (uint64_t)wd * deal.per + lane;
        uint32_t v = 0, beg = 0, end = 0;
        unsigned long long own = kSccDead;
        if (lane < deal.per && i < count) {
            v = list[i];
            own = ga_load(a.colour + v);
        }
        if (own != kSccDead) {
            beg = a.in_ptr[v] - a.in_base;
            end = a.in_ptr[v + 1u] - a.in_base;
        }
        unsigned long long best = own;                            // a dead predecessor's word is the largest: the minimum skips it
        rows_walk_thread(a.in_idx, beg, end, deal.steps, [&](const uint32_t(&c)[4], uint32_t) {
            unsigned long long k[4];
#pragma unroll
            for (int u = 0; u < 4; u++) k[u] = c[u] < a.n ? ga_load(a.colour + c[u]) : kSccDead;
            best = min(best, min(min(k[0], k[1]), min(k[2], k[3])));
            return false;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            unsigned long long low = kSccDead;
            rows_walk_wave(a.in_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t) {
                unsigned long long k[4];
#pragma unroll
                for (int u = 0; u < 4; u++) k[u] = c[u] < a.n ? ga_load(a.colour + c[u]) : kSccDead;
                low = min(low, min(min(k[0], k[1]), min(k[2], k[3])));
                return false;
            });
            low = scc_wave_min(low);
            if ((int)lane == src) best = min(best, low);          // (what its own thread found before the cut stays in)
        });
        if (best < own) {                                         // (own is not dead then: v owns the word, one store per row)
            ga_store(a.colour + v, best);
            changed += 1u;
        }
    }
    scc_count(a.ctl + kSccChanged, changed, lane);
}

__device__ __forceinline__ void scc_backward(const SccArgs &a, const uint32_t *list, uint32_t count, uint32_t lane, uint32_t wave) {
    const SccDeal deal = scc_deal(count, a.cut_steps);
    // w is the root of the colour x, or was found to reach it
    auto reaches = [&](uint32_t c, uint32_t, uint32_t x) { return c < a.n && (c == x || ga_load(a.mark + c) == x); };
    uint32_t changed = 0;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < deal.words; wd += gridDim.x * 4u) {
        const uint64_t i = (uint64_t)wd * deal.per + lane;
        uint32_t v = 0, cv = 0, beg = 0, end = 0;
        if (lane < deal.per && i < count) {
            v = list[i];
            const unsigned long long own = a.colour[v];           // (plain: forward's launches wrote it)
            cv = (uint32_t)own;
            if (own != kSccDead && cv != v && ga_load(a.mark + v) != cv) {
                beg = a.out_ptr[v] - a.out_base;
                end = a.out_ptr[v + 1u] - a.out_base;
            }
        }
        if (scc_row_any(a.out_idx, beg, end, deal.steps, lane, v, cv, reaches)) {
            ga_store(a.mark + v, cv);
            changed += 1u;
        }
    }
    scc_count(a.ctl + kSccChanged, changed, lane);
}

// roots and marked vertices are given to their component; the others start the next pass with their own key
__device__ __forceinline__ void scc_collect(const SccArgs &a, const uint32_t *list, uint32_t count, uint32_t lane) {
    uint32_t *next = a.lists + (size_t)(a.ctl[kSccWhich] ^ 1u) * a.n;
    const uint64_t nround = ((uint64_t)count + 255u) & ~255ull;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < nround; i += gridDim.x * 256u) {
        uint32_t v = 0;
        bool stays = false;
        if (i < count) {
            v = list[i];
            const unsigned long long own = a.colour[v];
            const uint32_t cv = (uint32_t)own;
            if (own != kSccDead) {
                stays = cv != v && a.mark[v] != cv;
                a.colour[v] = stays ? scc_key(a, v) : kSccDead;
                if (!stays) a.root[v] = cv;
            }
        }
        const uint32_t at = wave_append(stays, a.ctl + kSccNext, lane);
        if (stays && at < a.n) next[at] = v;                      // (at < n: a vertex is listed once)
    }
}

// the work of the phase the record names, over this pass's list
__global__ __launch_bounds__(256) void scc_round_kernel(SccArgs a) {
    const uint32_t phase = a.ctl[kSccPhase];
    if (phase == kSccDone || phase == kSccBegin) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t count = min(a.ctl[kSccCount], a.n);
    const uint32_t *list = a.lists + (size_t)(a.ctl[kSccWhich] & 1u) * a.n;
    if (phase == kSccTrim) scc_trim(a, list, count, lane, wave);
    else if (phase == kSccForward) scc_forward(a, list, count, lane, wave);
    else if (phase == kSccBackward) scc_backward(a, list, count, lane, wave);
    else if (phase == kSccCollect) scc_collect(a, list, count, lane);
}

// behind the begin and behind every round launch (plain loads and stores: a launch of its own)
__global__ void scc_turn_kernel(uint32_t *ctl, uint32_t n) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const uint32_t phase = ctl[kSccPhase];
    if (phase == kSccDone) return;
    const uint32_t changed = ctl[kSccChanged];
    ctl[kSccChanged] = 0u;
    *reinterpret_cast<unsigned long long *>(ctl + kSccSteps) += 1ull;
    bool new_pass = false;
    if (phase == kSccBegin) {
        ctl[kSccTrimmed] = changed;
        new_pass = true;
    } else if (phase == kSccCollect) {
        new_pass = true;
    } else {
        *reinterpret_cast<unsigned long long *>(ctl + kSccRounds) += 1ull;
        if (phase == kSccTrim) {
            const uint32_t alive = ctl[kSccAlive] - min(changed, ctl[kSccAlive]);
            ctl[kSccTrimmed] += changed;
            ctl[kSccAlive] = alive;
            if (alive == 0u) {
                ctl[kSccPhase] = kSccDone;
            } else if (changed == 0u) {
                ctl[kSccPasses] += 1u;
                ctl[kSccPhase] = kSccForward;
            }
        } else if (changed == 0u) {
            ctl[kSccPhase] = phase + 1u;                          // forward -> backward -> collect
        }
    }
    if (new_pass) {
        const uint32_t next = min(ctl[kSccNext], n);
        ctl[kSccNext] = 0u;
        ctl[kSccWhich] ^= 1u;
        ctl[kSccCount] = next;
        ctl[kSccAlive] = next;
        ctl[kSccPhase] = next != 0u ? kSccTrim : kSccDone;
    }
}

// the closing launches: they run once, in the batch whose turn said done
__global__ __launch_bounds__(256) void scc_min_kernel(const uint32_t *__restrict__ root, uint32_t *minv, uint32_t n, uint32_t *ctl) {
    if (ctl[kSccPhase] != kSccDone) return;
    uint32_t roots = 0;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t r = root[v];
        roots += r == (uint32_t)v ? 1u : 0u;
        if ((uint32_t)v < r && r < n) ga_min(minv + r, (uint32_t)v);
    }
    scc_count(ctl + kSccComponents, roots, threadIdx.x & 63u);
}

__global__ __launch_bounds__(256) void scc_label_kernel(uint32_t *__restrict__ label, const uint32_t *__restrict__ minv, uint32_t n,
                                                        const uint32_t *__restrict__ ctl) {
    if (ctl[kSccPhase] != kSccDone) return;
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t r = label[v];
        if (r < n) label[v] = minv[r];
    }
}

// the words of plan_in's scratch: the control record, colour (64 bits a vertex), then mark, minv and the two lists
constexpr size_t scc_scratch_bytes(size_t n) { return kRoundsCtlBytes + 24u * n; }

static int scc(gl_spmv_plan pin, gl_spmv_plan pout, const uint32_t *d_prio, uint32_t *d_label, uint64_t *h_stats, const char *who) {
    int rc = rows_require_pair(pin, pout, who, "io.simple_pattern");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = pin->num_rows;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = h_stats[4] = 0u;
    if (n == 0u) return GL_OK;
    if (pin->nnz == 0) {                                          // no entries: every vertex is a component of its own
        if ((rc = rows_iota(d_label, n)) != GL_OK) return rc;
        GL_HIP(hipStreamSynchronize(s));
        if (h_stats) h_stats[0] = n;
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 24): scc_cut = entries a thread reads before the wavefront
    // takes the row over, scc_grid = workgroups per compute unit of a round launch, scc_batch = (round, turn) pairs enqueued
    // between two read-backs of the control record
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("scc_cut", 8), 1l << 30, debug_knob("scc_grid", 4));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("scc_batch", 32), 4096));
    rc = plan_scratch(pin->d_scc_scratch, scc_scratch_bytes(n), who, "control record, colours, marks, minima and two vertex lists");
    if (rc != GL_OK) return rc;
    SccArgs a;
    a.in_ptr = pin->d_csr_indptr;
    a.in_idx = pin->d_csr_indices;
    a.in_base = pin->csr_nz_base;
    a.out_ptr = pout->d_csr_indptr;
    a.out_idx = pout->d_csr_indices;
    a.out_base = pout->csr_nz_base;
    a.prio = d_prio;
    a.ctl = reinterpret_cast<uint32_t *>(pin->d_scc_scratch);
    a.colour = reinterpret_cast<unsigned long long *>(pin->d_scc_scratch + kRoundsCtlBytes);
    a.root = d_label;
    a.mark = reinterpret_cast<uint32_t *>(a.colour + n);
    a.minv = a.mark + n;
    a.lists = a.minv + n;
    a.n = n;
    a.cut_steps = shape.cut_steps;
    const unsigned stream_grid = rows_stream_grid(n), round_grid = shape.grid;
    static_assert((kSccRecordWords + 1u) * 4u <= 64u && (kSccComponents + 1u) * 4u <= kRoundsCtlBytes,
                  "the record and the component count fit the page-locked staging words");
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    uint32_t seen[kSccRecordWords];                               // the record as the batch before left it
    for (uint32_t i = 0; i < kSccRecordWords; i++) seen[i] = w[i] = 0u;
    GL_HIP(hipMemsetAsync(a.ctl, 0, kRoundsCtlBytes, s));
    scc_begin_kernel<<<stream_grid, 256, 0, s>>>(a);
    scc_turn_kernel<<<1, 64, 0, s>>>(a.ctl, n);
    GL_LAUNCH_CHECK();
    uint64_t launches = 2;
    const uint64_t n64 = n, cap = n64 >= (1ull << 31) ? ~0ull : n64 * n64 + 6u * n64 + 8u;
    bool stuck = false;
    rc = rounds_run(
        batch, cap, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                scc_round_kernel<<<round_grid, 256, 0, s>>>(a);
                scc_turn_kernel<<<1, 64, 0, s>>>(a.ctl, n);
            }
            scc_min_kernel<<<stream_grid, 256, 0, s>>>(a.root, a.minv, n, a.ctl);
            scc_label_kernel<<<stream_grid, 256, 0, s>>>(d_label, a.minv, n, a.ctl);
            return 2ull * batch + 2ull;
        },
        [&] {
            const hipError_t e = hipMemcpyAsync(w, a.ctl, kSccRecordWords * 4u, hipMemcpyDeviceToHost, s);
            return e != hipSuccess ? e : hipMemcpyAsync(w + kSccRecordWords, a.ctl + kSccComponents, 4u, hipMemcpyDeviceToHost, s);
        },
        [&] {
            if (w[kSccPhase] == kSccDone) return kRoundsDone;
            stuck = true;
            for (uint32_t i = 0; i < kSccRecordWords; i++) {
                stuck = stuck && seen[i] == w[i];
                seen[i] = w[i];
            }
            return stuck ? kRoundsStuck : kRoundsGoOn;
        },
        [&](uint64_t steps) {
            return set_error(GL_ERR_HIP, "%s: internal error: %s after %llu steps on %u vertices (phase %u, pass %u, %u vertices listed, %u live)",
                             who, stuck ? "a batch did not move the control record" : "not done", (unsigned long long)steps, n, w[kSccPhase],
                             w[kSccPasses], w[kSccCount], w[kSccAlive]);
        });
    if (rc != GL_OK) return rc;
    if (h_stats) {
        h_stats[0] = w[kSccRecordWords];
        h_stats[1] = w[kSccPasses];
        h_stats[2] = w[kSccTrimmed];
        h_stats[3] = (uint64_t)w[kSccRounds] | ((uint64_t)w[kSccRounds + 1u] << 32);
        h_stats[4] = launches;
    }
    return GL_OK;
}

}  // namespace gl

int gl_scc(gl_spmv_plan plan_in, gl_spmv_plan plan_out, const uint32_t *d_prio, uint32_t *d_label, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan_in != nullptr && plan_out != nullptr && d_label != nullptr);
    GL_ARG(d_prio != d_label);
    return gl::scc(plan_in, plan_out, d_prio, d_label, h_stats, "gl_scc");
}
