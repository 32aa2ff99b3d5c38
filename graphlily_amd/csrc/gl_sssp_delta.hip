// Shortest paths by delta-stepping (gl_sssp_delta; Meyer and Sanders), run to convergence on the device over the plain CSR copies
// that two GL_PLAN_BOOLEAN plans keep (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base) -- plan_in, whose row v lists
// the PREDECESSORS of v (an entry A[v, u] is an edge u -> v), and plan_out, the transposed pattern's plan, whose row u lists its
// SUCCESSORS (plan_out == plan_in: a symmetric pattern) -- with an f32 weight per entry of each copy, on n = num_rows vertices.
//
//   dist[v]   = the least fixed point of d[s] = +0 on the sources, d[v] = min over the entries A[v, u] of (float)(d[u] + w); the
//               bits 0x7f800000 when unreached.  x -> (float)(x + w) is monotone and w >= 0, so the fixed point is unique and is
//               what Dijkstra's algorithm computes in f32 -- whatever delta, the schedule and the knobs.
//   parent[v] = v on a source, the smallest u with d[u] < d[v] and (float)(d[u] + w) == d[v] elsewhere, 0xffffffff without one
//
// DISTANCES live as their u32 bit patterns (d_dist itself): non-negative floats order as their bits do, so a relaxation is ONE
// atomic min that returns the word's value before, and "old > new" -- strictly -- is the only thing that ever queues a vertex:
// an edge of weight 0, a cycle of them, or a weight below the spacing of f32 at d (trap 2 of the issue) lowers nothing and
// queues nothing.  A sum that overflows to +inf is dropped before the atomic.  The vertex whose atomic finds 0x7f800000 is the one
// that reaches it: `reached` counts those.
// BUCKETS: bucket(d) = min((uint32_t)(d * (1 / delta)), 2^30) -- only its monotonicity is used.  An edge is LIGHT when w < delta.
//
// STATE, all of it O(n) words behind plan_in: two QUEUES (this round's, the next round's), two FAR PILES (the
// pile, and the one a split compacts it into), the bucket's SETTLED list, and per vertex
//   qstamp[v] = the last round (a serial number) in which v was appended to the next queue
//   rstamp[v] = the last bucket visit (an epoch number) in which v was appended to the settled list
//   pstamp[v] = 1 while v is in the far pile
//   last[v]   = the distance bits v was last expanded at (0xffffffff: never)
// A vertex is appended to a list only by the thread that moved its stamp, so every list holds a vertex at most once and at most n
// words: no list can overflow, whatever the graph (the stores keep a bound check all the same).
// INVARIANT between launches: a vertex whose distance was lowered after its last expansion is in the queue or in the pile.
// PHASES, one control record {phase, bucket, queue, count, pile, serial, epoch, rounds, done}:
//   LIGHT  a round over the queue: every queued v reads d = dist[v], notes last[v] = d, joins the settled list (once per epoch)
//          and relaxes the light entries of row v of plan_out.  A vertex whose distance drops goes to the next queue when its new
//          bucket is the current one, else to the pile.  The turn behind it swaps the queues, or, the next one being empty,
//          moves on to HEAVY (delta = +inf: to SCAN).
//   HEAVY  one pass over the settled list: the heavy entries, from the final distances of the bucket; everything lowered goes to
//          the pile, the current bucket's own included -- in the clamped top bucket, or where the spacing of f32 exceeds delta, a
//          heavy edge need not leave the bucket (trap 1).
//   SCAN   over the pile: the smallest bucket among the entries whose distance is not the one they were last expanded at (the
//          others are stale: expanded since they were piled).  None: done.
//   SPLIT  over the pile: the entries of that bucket become the queue, the stale ones are dropped, the rest are compacted into
//          the other pile; the turn behind it starts a new epoch, so that the settled list starts afresh even when the bucket is
//          the one just left.  Empty buckets are never visited one by one.
// Both LIGHT and HEAVY are sssp_round_kernel, the walk of gl_rows.h: a thread per listed vertex, the weight loads issued with the
// index loads; the wavefront takes over a row still unfinished after sssp_delta_cut = 8 entries, 256 entries a step; a wavefront
// that holds ONE vertex hands the row to all lanes at once.  The thread steps are a copy of rows_walk_thread in which EVERY lane
// takes every step (as match_collect_kernel's), so that they too append with wave_append: one atomic per wavefront, list and entry
// slot, wherever a vertex is appended.
// MEMORY RULE and GATING: gl_rounds.h.  Atomic-only inside a round launch: dist[], qstamp[], rstamp[], pstamp[] and the tails.
// last[], the lists and the record are written by one launch and read by later ones; SCAN and SPLIT read dist[] plainly, no launch
// of theirs writes it.  The host enqueues (round, turn, pile, turn, pile, turn) x sssp_delta_batch blindly; a launch whose phase is
// not on returns at once.  No spin-wait, no float atomic.
// STEP CAP.  Every candidate a launch forms is (float)(d + w) >= d for the distance d of a LIVE vertex (queued, or in the pile and
// not stale), and only a strictly smaller candidate makes a vertex live again.
//   Rounds of one epoch <= n.  The light rounds of an epoch form candidates from queued vertices only, so the queued vertex of
//     smallest distance is not lowered again IN THIS EPOCH -- every candidate is at least its distance -- and is not queued again
//     in it: every round that runs retires another vertex for the epoch.
//   Epochs <= n.  When an epoch starts, the live vertex of smallest distance lies in the chosen bucket, hence in the queue, and
//     nothing anywhere can lower it any more: it is FINAL.  The epoch expands it at that distance, light entries in a round and
//     heavy entries in the HEAVY pass, so it is never live again: every epoch retires a vertex for good.  (SCAN finds a live entry
//     or ends the run, so every SPLIT leaves a queue that is not empty.)
// "The smallest queued vertex is final" does NOT hold across epochs: heavy entries wait for the end of the epoch, and where a heavy
// edge stays in its bucket (trap 1) it re-opens vertices the light rounds had settled, and a whole chain of light rounds with
// them -- k heavy edges into the head of a zero-weight chain of m vertices cost about k (m + 1) steps.  Every step of six launches
// runs a round or a HEAVY pass, but the first, which only splits the sources off: at most n (n + 1) + 1 steps, capped at
// n (n + 1) + 4.  Where every heavy edge leaves its bucket -- any delta above f32's spacing at the distances met, below the clamp --
// a vertex final in its epoch is final, and the run takes at most 2 n + 1 steps.  The cap keeps a wrong build that still moves
// from running for ever; one that does not move is caught at once: a batch that leaves the record as it was is an internal error.
// STATS: reached is a function of the input.  Rounds and relaxations depend on the order in which the atomics of a launch are
// served (a round may carry a distance over several edges), and buckets with them where a heavy edge stays in its bucket.
#include "gl_rounds.h"
#include "graphlily_hip_sssp_delta.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace gl {

// the control record (words); what the launches between two turns add to sits in the second 128-byte line
enum : uint32_t { kSsspPhase = 0, kSsspBucket = 1, kSsspQCur = 2, kSsspQCount = 3, kSsspPCur = 4, kSsspSerial = 5, kSsspEpoch = 6,
                  kSsspRounds = 7, kSsspDone = 8, kSsspRecordWords = 9,
                  kSsspQTail = 32, kSsspPTail = 33, kSsspRTail = 34, kSsspP2Tail = 35, kSsspBest = 36,
                  kSsspLowered = 38 /* 64 bits */, kSsspReached = 40, kSsspCounterWords = 3 };
enum : uint32_t { kSsspScan = 0, kSsspSplit = 1, kSsspLight = 2, kSsspHeavy = 3 };      // (a zeroed record starts with SCAN)
enum : uint32_t { kSsspNone = 0, kSsspToQueue = 1, kSsspToPile = 2 };
constexpr uint32_t kSsspInf = 0x7f800000u;       // the dist bits of an unreached vertex
constexpr uint32_t kSsspNoParent = 0xffffffffu;  // ... its parent, and the `last` of a vertex never expanded
constexpr uint32_t kSsspTop = 1u << 30;          // the clamped top bucket

// monotone in d >= 0, whatever inv (0 for delta = +inf; +inf, with its NaN at d = 0, for a subnormal delta)
__device__ __forceinline__ uint32_t sssp_bucket(uint32_t bits, float inv) {
    const float q = __uint_as_float(bits) * inv;
    return q < (float)kSsspTop ? (uint32_t)q : kSsspTop;
}
__device__ __forceinline__ uint32_t sssp_wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += (uint32_t)__shfl_xor((int)x, d);
    return x;
}

struct SsspArgs {
    const uint32_t *out_ptr, *out_idx;
    const float *weight_out;
    uint32_t *dist, *parent;                       // (the bits of d_dist)
    uint32_t *ctl, *queue, *pile;                  // queue / pile: two buffers of n words each, one behind the other
    uint32_t *settled, *qstamp, *rstamp, *pstamp, *last;
    float delta, inv_delta;
    uint32_t n, out_base, cut_steps, has_heavy;
};

// distances, stamps and parents as a call finds them; the record was zeroed by a memset in front of this launch
__global__ __launch_bounds__(256) void sssp_fill_kernel(SsspArgs a) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < a.n; v += gridDim.x * 256u) {
        a.dist[v] = kSsspInf;
        a.qstamp[v] = a.rstamp[v] = a.pstamp[v] = 0u;
        a.last[v] = kSsspNoParent;
        if (a.parent) a.parent[v] = kSsspNoParent;
    }
}

// every source that is a vertex, once: distance 0, its own parent, a member of the pile (the first SCAN finds bucket 0)
__global__ __launch_bounds__(256) void sssp_sources_kernel(SsspArgs a, const uint32_t *__restrict__ sources, uint32_t k) {
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < k; i += gridDim.x * 256u) {
        const uint32_t s = sources[i];
        if (s >= a.n || ga_fetch_min(a.dist + s, 0u) != kSsspInf) continue;
        a.pstamp[s] = 1u;                                         // (plain: the one thread that reached s; nobody reads it now)
        if (a.parent) a.parent[s] = s;
        const uint32_t pos = ga_add(a.ctl + kSsspPTail, 1u);
        if (pos < a.n) a.pile[pos] = s;
        (void)ga_add(a.ctl + kSsspReached, 1u);
    }
}

// a plan without entries, or no sources: the sources that are vertices are reached, nothing else is.  One launch: every vertex
// looks itself up in the list.
__global__ __launch_bounds__(256) void sssp_flat_kernel(float *__restrict__ dist, uint32_t *__restrict__ parent,
                                                        const uint32_t *__restrict__ sources, uint32_t k, uint32_t n) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        bool is_source = false;
        for (uint32_t i = 0; i < k && !is_source; i++) is_source = sources[i] == (uint32_t)v;
        dist[v] = is_source ? 0.0f : __uint_as_float(kSsspInf);
        if (parent) parent[v] = is_source ? (uint32_t)v : kSsspNoParent;
    }
}

// The entry (c, w) of the row of a vertex at distance d: lower dist[c] to (float)(d + w) when the entry belongs to this pass.
// -> where the caller appends c: to the next queue, to the pile, or nowhere -- c was not lowered, or is in that list already.
__device__ __forceinline__ uint32_t sssp_relax(const SsspArgs &a, uint32_t c, float d, float w, bool heavy, uint32_t bucket, uint32_t serial,
                                               uint32_t &lowered, uint32_t &reached) {
    if (c >= a.n || (w < a.delta) == heavy) return kSsspNone;
    const uint32_t cand = __float_as_uint(d + w);
    if (cand >= kSsspInf) return kSsspNone;                       // the sum overflowed
    const uint32_t old = ga_fetch_min(a.dist + c, cand);
    if (old <= cand) return kSsspNone;                            // (strictly: zero weights and absorbed weights queue nothing)
    lowered += 1u;
    reached += old == kSsspInf ? 1u : 0u;
    if (!heavy && sssp_bucket(cand, a.inv_delta) == bucket) return ga_fetch_max(a.qstamp + c, serial) < serial ? kSsspToQueue : kSsspNone;
    return ga_fetch_max(a.pstamp + c, 1u) == 0u ? kSsspToPile : kSsspNone;
}

__global__ __launch_bounds__(256) void sssp_round_kernel(SsspArgs a) {
    if (a.ctl[kSsspDone] != 0u) return;
    const uint32_t phase = a.ctl[kSsspPhase];
    if (phase != kSsspLight && phase != kSsspHeavy) return;
    const bool heavy = phase == kSsspHeavy;
    const uint32_t bucket = a.ctl[kSsspBucket], serial = a.ctl[kSsspSerial], epoch = a.ctl[kSsspEpoch];
    const uint32_t *items = heavy ? a.settled : a.queue + (size_t)a.ctl[kSsspQCur] * a.n;
    uint32_t *next = a.queue + (size_t)(a.ctl[kSsspQCur] ^ 1u) * a.n, *pile = a.pile + (size_t)a.ctl[kSsspPCur] * a.n;
    const uint32_t count = heavy ? min(a.ctl[kSsspRTail], a.n) : a.ctl[kSsspQCount];      // (no launch of HEAVY appends to the settled list)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * 4u;
    // listed vertices per wavefront: 64, fewer when the list is shorter than the launch; a wavefront with ONE vertex gives its
    // row to all lanes at once (topo_round_kernel's dealing)
    const uint32_t per = min(64u, max(1u, (uint32_t)(((uint64_t)count + nwaves - 1u) / nwaves)));
    const uint32_t nwords = (uint32_t)(((uint64_t)count + per - 1u) / per);
    const uint32_t thread_steps = per == 1u ? 0u : a.cut_steps;
    uint32_t lowered = 0u, reached = 0u;
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t item = (uint64_t)wd * per + lane;
        const bool in = lane < per && item < count;
        uint32_t v = 0u, beg = 0u, end = 0u;
        float d = 0.0f;
        if (in) {
            v = items[item];
            const uint32_t bits = ga_load(a.dist + v);
            d = __uint_as_float(bits);
            beg = a.out_ptr[v] - a.out_base;
            end = a.out_ptr[v + 1u] - a.out_base;
            if (!heavy) a.last[v] = bits;                         // (one writer: a queue holds v once)
        }
        if (!heavy && a.has_heavy != 0u) {                        // settled in this bucket: the HEAVY pass will expand it
            const bool hit = in && ga_fetch_max(a.rstamp + v, epoch) < epoch;
            const uint32_t pos = wave_append(hit, a.ctl + kSsspRTail, lane);
            if (hit && pos < a.n) a.settled[pos] = v;
        }
        // rows_walk_thread with every lane in every step (a lane whose row is finished holds four paddings): wave_append needs them all
        for (uint32_t step = 0; step < thread_steps && __any(beg < end); step++) {
            uint32_t c[4], to[4];
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) c[u] = end - beg > (uint32_t)u ? a.out_idx[beg + u] : 0xffffffffu;
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = end - beg > (uint32_t)u ? a.weight_out[beg + u] : 0.0f;
#pragma unroll
            for (int u = 0; u < 4; u++) to[u] = sssp_relax(a, c[u], d, w[u], heavy, bucket, serial, lowered, reached);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t qpos = wave_append(to[u] == kSsspToQueue, a.ctl + kSsspQTail, lane);
                if (to[u] == kSsspToQueue && qpos < a.n) next[qpos] = c[u];
                const uint32_t ppos = wave_append(to[u] == kSsspToPile, a.ctl + kSsspPTail, lane);
                if (to[u] == kSsspToPile && ppos < a.n) pile[ppos] = c[u];
            }
            beg += min(4u, end - beg);
        }
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const float row_d = __shfl(d, src);
            rows_walk_wave(a.out_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
                float w[4];
                uint32_t to[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint64_t j = base + 64u * u + lane;
                    w[u] = j < e ? a.weight_out[j] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) to[u] = sssp_relax(a, c[u], row_d, w[u], heavy, bucket, serial, lowered, reached);
#pragma unroll
                for (int u = 0; u < 4; u++) {                     // (every lane is here: one atomic add per wavefront, list and step)
                    const uint32_t qpos = wave_append(to[u] == kSsspToQueue, a.ctl + kSsspQTail, lane);
                    if (to[u] == kSsspToQueue && qpos < a.n) next[qpos] = c[u];
                    const uint32_t ppos = wave_append(to[u] == kSsspToPile, a.ctl + kSsspPTail, lane);
                    if (to[u] == kSsspToPile && ppos < a.n) pile[ppos] = c[u];
                }
                return false;
            });
        });
    }
    lowered = sssp_wave_sum(lowered);
    reached = sssp_wave_sum(reached);
    if (lane == 0u && lowered != 0u) {
        ga_add(reinterpret_cast<unsigned long long *>(a.ctl + kSsspLowered), (unsigned long long)lowered);
        if (reached != 0u) (void)ga_add(a.ctl + kSsspReached, reached);
    }
}

// SCAN and SPLIT: a thread per entry of the pile, whole wavefronts on every trip
__global__ __launch_bounds__(256) void sssp_pile_kernel(SsspArgs a) {
    if (a.ctl[kSsspDone] != 0u) return;
    const uint32_t phase = a.ctl[kSsspPhase];
    if (phase != kSsspScan && phase != kSsspSplit) return;
    const uint32_t chosen = a.ctl[kSsspBucket], count = min(a.ctl[kSsspPTail], a.n), lane = threadIdx.x & 63u;
    const uint32_t *pile = a.pile + (size_t)a.ctl[kSsspPCur] * a.n;
    uint32_t *stays = a.pile + (size_t)(a.ctl[kSsspPCur] ^ 1u) * a.n, *queue = a.queue + (size_t)a.ctl[kSsspQCur] * a.n;
    const uint64_t nround = ((uint64_t)count + 255u) & ~255ull;
    uint32_t best = 0u;                                           // the largest ~bucket: 0 = no live entry (a bucket is <= 2^30)
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < nround; i += gridDim.x * 256u) {
        const bool in = i < count;
        const uint32_t v = in ? pile[i] : 0u;
        const uint32_t bits = in ? a.dist[v] : 0u;
        const bool live = in && bits != a.last[v];                // (stale: expanded at this very distance since it was piled)
        const uint32_t b = sssp_bucket(bits, a.inv_delta);
        if (phase == kSsspScan) {
            if (live) best = max(best, ~b);
            continue;
        }
        const bool go = live && b <= chosen, stay = live && !go;
        const uint32_t qpos = wave_append(go, a.ctl + kSsspQTail, lane);
        if (go && qpos < a.n) queue[qpos] = v;
        const uint32_t ppos = wave_append(stay, a.ctl + kSsspP2Tail, lane);
        if (stay && ppos < a.n) stays[ppos] = v;
        if (in && !stay) a.pstamp[v] = 0u;                        // (one writer: the pile holds v once)
    }
    if (phase == kSsspScan) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) best = max(best, (uint32_t)__shfl_xor((int)best, d));
        if (lane == 0u && best != 0u) ga_max(a.ctl + kSsspBest, best);
    }
}

// behind a round (after_round) or a pile launch: one thread, plain loads and stores, a launch of its own.  It acts on the phases
// of the launch in front of it only, which found the same record.
__global__ void sssp_turn_kernel(uint32_t *ctl, uint32_t n, uint32_t after_round, uint32_t has_heavy) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    if (ctl[kSsspDone] != 0u) return;
    const uint32_t phase = ctl[kSsspPhase];
    if (after_round != 0u && phase == kSsspLight) {
        const uint32_t next = min(ctl[kSsspQTail], n);
        ctl[kSsspRounds] += 1u;
        if (next != 0u) {
            ctl[kSsspQCur] ^= 1u;
            ctl[kSsspQCount] = next;
            ctl[kSsspQTail] = 0u;
            ctl[kSsspSerial] += 1u;
        } else {
            ctl[kSsspPhase] = has_heavy != 0u ? kSsspHeavy : kSsspScan;
        }
    } else if (after_round != 0u && phase == kSsspHeavy) {
        ctl[kSsspPhase] = kSsspScan;
    } else if (after_round == 0u && phase == kSsspScan) {
        const uint32_t best = ctl[kSsspBest];
        if (best == 0u) {
            ctl[kSsspDone] = 1u;                                  // nothing live is left anywhere
        } else {
            ctl[kSsspBucket] = ~best;                             // (may be the bucket just left: trap 1)
            ctl[kSsspBest] = 0u;
            ctl[kSsspPhase] = kSsspSplit;
        }
    } else if (after_round == 0u && phase == kSsspSplit) {
        ctl[kSsspPCur] ^= 1u;
        ctl[kSsspPTail] = min(ctl[kSsspP2Tail], n);
        ctl[kSsspP2Tail] = 0u;
        ctl[kSsspQCount] = min(ctl[kSsspQTail], n);               // (SPLIT filled the current queue)
        ctl[kSsspQTail] = 0u;
        ctl[kSsspRTail] = 0u;                                     // the settled list starts afresh
        ctl[kSsspEpoch] += 1u;
        ctl[kSsspSerial] += 1u;
        ctl[kSsspPhase] = kSsspLight;
    }
}

// SSSP.parents()'s definition by one pull over plan_in: a thread per vertex, the wavefront behind it; the columns ascend, so the
// first entry that fits is the smallest.  Sources hold themselves already, every other word 0xffffffff.
__global__ __launch_bounds__(256) void sssp_parent_kernel(const uint32_t *__restrict__ in_ptr, const uint32_t *__restrict__ in_idx,
                                                          uint32_t in_base, const float *__restrict__ weight, const float *__restrict__ dist,
                                                          uint32_t *__restrict__ parent, uint32_t n, uint32_t cut_steps) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * 4u, nwords = (uint32_t)(((uint64_t)n + 63u) / 64u);
    for (uint32_t wd = blockIdx.x * 4u + wave; wd < nwords; wd += nwaves) {
        const uint64_t v64 = (uint64_t)wd * 64u + lane;
        const uint32_t v = (uint32_t)v64;
        float dv = 0.0f;
        uint32_t beg = 0u, end = 0u, best = kSsspNoParent;
        bool want = false;
        if (v64 < n) {
            dv = dist[v];
            want = __float_as_uint(dv) < kSsspInf && parent[v] != v;
            if (want) {
                beg = in_ptr[v] - in_base;
                end = in_ptr[v + 1u] - in_base;
            }
        }
        rows_walk_thread(in_idx, beg, end, cut_steps, [&](const uint32_t(&c)[4], uint32_t at) {
            float w[4], du[4];
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = end - at > (uint32_t)u ? weight[at + u] : 0.0f;
#pragma unroll
            for (int u = 0; u < 4; u++) du[u] = c[u] < n ? dist[c[u]] : 0.0f;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (best == kSsspNoParent && c[u] < n && du[u] < dv && du[u] + w[u] == dv) best = c[u];
            return best != kSsspNoParent;
        });
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const float row_d = __shfl(dv, src);
            uint32_t m = kSsspNoParent;
            rows_walk_wave(in_idx, b, e, lane, [&](const uint32_t(&c)[4], uint64_t base) {
                float w[4], du[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint64_t j = base + 64u * u + lane;
                    w[u] = j < e ? weight[j] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) du[u] = c[u] < n ? dist[c[u]] : 0.0f;
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (c[u] < n && du[u] < row_d && du[u] + w[u] == row_d) m = min(m, c[u]);
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) m = min(m, (uint32_t)__shfl_xor((int)m, d));
                return m != kSsspNoParent;                        // (the same in every lane; later steps hold larger columns)
            });
            if ((int)lane == src) best = m;
        });
        if (want) parent[v] = best;
    }
}

// the words of plan_in's scratch: the control record, then the nine arrays
constexpr size_t sssp_scratch_bytes(size_t n) { return kRoundsCtlBytes + 36u * n; }

static int sssp_delta(gl_spmv_plan pin, gl_spmv_plan pout, const float *d_weight_in, const float *d_weight_out, const uint32_t *d_sources,
                      uint32_t num_sources, float delta, float *d_dist, uint32_t *d_parent, uint64_t *h_stats, const char *who) {
    int rc = rows_require_pair(pin, pout, who, "io.directed_weighted");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = pin->num_rows;
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = h_stats[4] = 0u;
    if (n == 0u) return GL_OK;
    // the outputs are distinct arrays of n words, and neither is a weight array
    {
        const size_t bytes = 4u * (size_t)n, wbytes = 4u * (size_t)pin->nnz;
        const char *p = (const char *)d_dist, *q = (const char *)d_parent;
        if (q && p < q + bytes && q < p + bytes) return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: two output arrays overlap", who);
        for (const char *out : {p, q})
            for (const char *w : {(const char *)d_weight_in, (const char *)d_weight_out})
                if (out && wbytes && out < w + wbytes && w < out + bytes)
                    return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: an output array overlaps a weight array", who);
    }
    const unsigned stream_grid = rows_stream_grid(n);
    if (pin->nnz == 0 || num_sources == 0u) {                     // nothing to relax: the sources, and nobody else
        sssp_flat_kernel<<<stream_grid, 256, 0, s>>>(d_dist, d_parent, d_sources, num_sources, n);
        GL_LAUNCH_CHECK();
        std::vector<uint32_t> src(num_sources);
        if (num_sources) GL_HIP(hipMemcpyAsync(src.data(), d_sources, 4u * (size_t)num_sources, hipMemcpyDeviceToHost, s));
        GL_HIP(hipStreamSynchronize(s));
        std::sort(src.begin(), src.end());
        src.erase(std::unique(src.begin(), src.end()), src.end());
        if (h_stats) {
            h_stats[0] = (uint64_t)(std::lower_bound(src.begin(), src.end(), n) - src.begin());
            h_stats[4] = 1u;
        }
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 34): sssp_delta_cut = entries a thread reads of a row before
    // the wavefront takes it over, sssp_delta_grid = workgroups per compute unit of a round launch, sssp_delta_batch = steps of
    // six launches enqueued between two read-backs of the control record.  gl_topo's cut and grid; a quarter of its batch,
    // a step being three times as many launches.  Guesses until measured.
    const RowsWalkShape shape = rows_walk_shape(n, debug_knob("sssp_delta_cut", 8), 1l << 30, debug_knob("sssp_delta_grid", 4));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("sssp_delta_batch", 16), 4096));
    rc = plan_scratch(pin->d_sssp_delta_scratch, sssp_scratch_bytes(n), who, "control record, queues, piles, settled list and stamps");
    if (rc != GL_OK) return rc;
    SsspArgs a;
    a.out_ptr = pout->d_csr_indptr;
    a.out_idx = pout->d_csr_indices;
    a.out_base = pout->csr_nz_base;
    a.weight_out = d_weight_out;
    a.dist = reinterpret_cast<uint32_t *>(d_dist);
    a.parent = d_parent;
    a.ctl = reinterpret_cast<uint32_t *>(pin->d_sssp_delta_scratch);
    a.queue = a.ctl + kRoundsCtlBytes / 4u;
    a.pile = a.queue + 2u * (size_t)n;
    a.settled = a.pile + 2u * (size_t)n;
    a.qstamp = a.settled + n;
    a.rstamp = a.qstamp + n;
    a.pstamp = a.rstamp + n;
    a.last = a.pstamp + n;
    a.delta = delta;
    a.inv_delta = 1.0f / delta;
    a.n = n;
    a.cut_steps = shape.cut_steps;
    a.has_heavy = std::isfinite(delta) ? 1u : 0u;
    const unsigned round_grid = shape.grid;
    constexpr uint32_t kWords = kSsspRecordWords + kSsspCounterWords;
    static_assert(kWords * 4u <= 64u, "the record and the counters fit the page-locked staging words");
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    uint32_t seen[kWords];                                        // the record as the batch before left it
    for (uint32_t i = 0; i < kWords; i++) seen[i] = w[i] = 0u;
    GL_HIP(hipMemsetAsync(a.ctl, 0, kRoundsCtlBytes, s));
    sssp_fill_kernel<<<stream_grid, 256, 0, s>>>(a);
    sssp_sources_kernel<<<std::max(1u, std::min(cdiv(num_sources, 256u), stream_grid)), 256, 0, s>>>(a, d_sources, num_sources);
    GL_LAUNCH_CHECK();
    uint64_t launches = 2;
    bool stuck = false;
    rc = rounds_run(
        batch, (uint64_t)n * ((uint64_t)n + 1ull) + 4ull, launches,      // the header's step cap (n < 2^32: no wrap)
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                sssp_round_kernel<<<round_grid, 256, 0, s>>>(a);
                sssp_turn_kernel<<<1, 64, 0, s>>>(a.ctl, n, 1u, a.has_heavy);
                for (int k = 0; k < 2; k++) {                     // SCAN, then SPLIT
                    sssp_pile_kernel<<<stream_grid, 256, 0, s>>>(a);
                    sssp_turn_kernel<<<1, 64, 0, s>>>(a.ctl, n, 0u, a.has_heavy);
                }
            }
            return 6ull * batch;
        },
        [&] {
            const hipError_t e = hipMemcpyAsync(w, a.ctl, kSsspRecordWords * 4u, hipMemcpyDeviceToHost, s);
            return e != hipSuccess ? e : hipMemcpyAsync(w + kSsspRecordWords, a.ctl + kSsspLowered, kSsspCounterWords * 4u, hipMemcpyDeviceToHost, s);
        },
        [&] {
            if (w[kSsspDone] != 0u) return kRoundsDone;
            stuck = true;
            for (uint32_t i = 0; i < kWords; i++) {
                stuck = stuck && seen[i] == w[i];
                seen[i] = w[i];
            }
            return stuck ? kRoundsStuck : kRoundsGoOn;
        },
        [&](uint64_t steps) {
            return set_error(GL_ERR_HIP, "%s: internal error: %s after %llu steps on %u vertices (phase %u, bucket %u, %u buckets visited, %u rounds)",
                             who, stuck ? "a batch did not move the control record" : "not done", (unsigned long long)steps, n, w[kSsspPhase],
                             w[kSsspBucket], w[kSsspEpoch], w[kSsspRounds]);
        });
    if (rc != GL_OK) return rc;
    if (d_parent) {
        sssp_parent_kernel<<<round_grid, 256, 0, s>>>(pin->d_csr_indptr, pin->d_csr_indices, pin->csr_nz_base, d_weight_in, d_dist, d_parent, n,
                                                      shape.cut_steps);
        GL_LAUNCH_CHECK();
        GL_HIP(hipStreamSynchronize(s));
        launches += 1;
    }
    if (h_stats) {
        h_stats[0] = w[kSsspRecordWords + 2u];
        h_stats[1] = w[kSsspEpoch];
        h_stats[2] = w[kSsspRounds];
        h_stats[3] = ((uint64_t)w[kSsspRecordWords + 1u] << 32) | w[kSsspRecordWords];
        h_stats[4] = launches;
    }
    return GL_OK;
}

}  // namespace gl

int gl_sssp_delta(gl_spmv_plan plan_in, gl_spmv_plan plan_out, const float *d_weight_in, const float *d_weight_out, const uint32_t *d_sources,
                  uint32_t num_sources, float delta, float *d_dist, uint32_t *d_parent, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan_in != nullptr && plan_out != nullptr && d_weight_in != nullptr && d_weight_out != nullptr && d_dist != nullptr);
    GL_ARG(d_sources != nullptr || num_sources == 0u);
    GL_ARG(delta > 0.0f);                                         // (false for NaN; +inf passes)
    return gl::sssp_delta(plan_in, plan_out, d_weight_in, d_weight_out, d_sources, num_sources, delta, d_dist, d_parent, h_stats, "gl_sssp_delta");
}
