// k-truss decomposition (gl_truss): level-synchronous EDGE peeling (PKT-style, after Kabir & Madduri) over the plain CSR
// copy that every GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base), on a square,
// whole-matrix plan whose rows are strictly ascending sets N(v) of columns below num_cols and whose pattern is SYMMETRIC.  An ENTRY
// is a stored (v, u); entry j is word j of the row copy.  An EDGE is the pair of entries (v, u), (u, v), u != v; there are m.
//
//   support[j] = |N(v) & N(u)| (without v and u themselves): the triangles through the edge
//   truss[j]   = the largest k such that the edge lies in a subgraph in which every edge is in >= k - 2 triangles of that subgraph
//                (an edge in no triangle: 2; both entries of an edge carry the same value; an entry (v, v): 0 in both arrays)
//
// EDGE NUMBERING (once per plan, cached in plan scratch): eid[j] in [0, m) numbers the entries with row < column in row order;
// the mirror entry (u, v), u > v, gets its partner's number through rows_lower_bound in row v.  esrc[e] / eent[e] give edge e's
// smaller end and its entry.  All state below is per edge.
// STATE: S[m], which starts as the support and ends as truss - 2 -- an edge's word is frozen at the level it is
// queued at; a QUEUE of m edge numbers, which every edge enters exactly once; pos[m], an edge's position in the queue
// (0xffffffff while it is not queued); and a CONTROL RECORD {l, lo, hi, phase, counters} + tail (a line of its own).
//   scan   (phase "scan")  appends every unqueued edge with S == l: one ballot and one atomic add to tail per wavefront; it also
//                          records the smallest S above l among the unqueued edges (one atomic min per wavefront)
//   peel   (phase "peel")  one SUB-ROUND over the queue slice [lo, hi) fixed at launch.  An edge's STATUS is read from pos alone:
//                          pos < lo: removed; lo <= pos < hi: in the slice; anything else -- the sentinel, or a position handed
//                          out during this very launch, which is >= hi -- later.  The status cannot change during a launch, so
//                          no decision races.  For a sliced edge e = (u, v) and every common neighbour w, e1 = (u, w), e2 = (v, w):
//                            either removed: skip (the triangle went when that edge was peeled); both in the slice: skip;
//                            exactly one, say e1, in the slice: decrement e2 iff e < e1 (of the two sliced edges of a triangle one
//                            takes the decrement); neither: decrement both
//                          decrement(x): a compare-and-swap loop that acts only while S[x] > l; the swap that writes l appends x
//                          and writes pos[x]
//   turn   (one thread)    lo = hi, hi = tail; a slice that is not empty is a sub-round; an empty one ends the level: phase =
//                          scan, and l += 1 -- or, when the level's scan found nobody, l = the smallest S it saw (EMPTY LEVELS
//                          are jumped over: nothing was decremented since that scan, so no edge lies between; the result does not
//                          depend on it, and `levels` counts the levels that removed an edge); tail == m: done (every edge still
//                          queued has its final word: the slice that completes the queue is never peeled)
// S == l IS REACHED EXACTLY ONCE per edge: S[x] is written only by successful swaps old -> old - 1 with old > l, so within a level it
// descends by single steps and never passes below l; every value is therefore written by at most one swap, and only the swap that
// writes l appends.  Across levels l only grows, and an edge at S == l is queued before l moves on (by that swap, or by the scan),
// after which its word is never written again: every swap needs S > l.  No transient dip, so the scan's plain loads see final words.
// BOTH passes over triangles give a GROUP of lanes (truss_group: 64, a wavefront) to an edge: the group walks the shorter of the
// two rows in coalesced pieces and looks every entry up in the longer one with rows_lower_bound.  A peel launch whose slice leaves
// half its threads idle doubles the lanes per edge until it does not, up to 1 << truss_spread (10) lanes across wavefronts and
// workgroups -- the peel reduces nothing, so a group need not share a wavefront: late sub-rounds hold a few hub edges, and one
// group walking a row of thousands of entries alone was the whole step (EXPERIMENTS.md Round 18: 4.5 times on the call).  Rows are
// not staged in LDS (gl_tc does): the edge (hub, hub) has two rows beyond any cap, and the variant was not built, so not measured.
// MEMORY RULE and GATING: gl_rounds.h.  Atomic-only inside a peel launch: S[], pos[] and the tail (rows, eid, the queue slice and
// the control record were written by earlier launches; queue words written now are read by later ones); inside a scan launch the
// tail and the record's `next` word, inside the support pass its 64-bit sum.  The host enqueues (scan, peel, turn) x truss_batch
// -- a scan that finds the phase "peel" returns at once and vice versa -- and then the pass that writes d_truss, gated on "done".
// At most m sub-rounds exist and at most max support + 1 <= m levels are scanned, so the loop is capped.
// The control record is gl_rounds.h's peel record (kPeelLevel = l, kPeelTop = the last level that removed an edge) and two
// words more: kTrussNext, and the 64-bit kTrussSum behind the tail in the second 128-byte line.
#include "gl_rounds.h"
#include "graphlily_hip_truss.h"

namespace gl {

constexpr uint32_t kTrNone = 0xffffffffu;

// the plan's cached part, then the words of one call
struct TrArgs {
    const uint32_t *row_ptr, *row_idx;
    const uint32_t *eid, *esrc, *eent;
    uint32_t *S, *queue, *pos, *ctl;
    uint32_t m, nz_base, g_shift, spread_shift;
};

// up[v] = entries of row v above the diagonal
__global__ __launch_bounds__(256) void truss_upper_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                          uint32_t n, uint32_t nz_base, uint32_t *__restrict__ up) {
    for (uint64_t v = blockIdx.x * 256u + threadIdx.x; v < n; v += gridDim.x * 256u) {
        const uint32_t b = row_ptr[v] - nz_base, len = row_ptr[v + 1u] - nz_base - b;
        uint32_t below = 0;
        if (len != 0u && (uint32_t)v + 1u < n) {
            const uint32_t at = rows_lower_bound(row_idx + b, len, (uint32_t)v + 1u);
            below = row_idx[b + at] > (uint32_t)v ? at : len;
        } else {
            below = len;                                             // (the last vertex has nobody above it)
        }
        up[v] = len - below;
    }
}

// off[0 .. n] = exclusive prefix sums of off[0 .. n), in place: one workgroup (once per plan)
__global__ __launch_bounds__(1024) void truss_offsets_kernel(uint32_t *off, uint32_t n) {
    __shared__ uint32_t wave_sum[16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < n; base += 1024u) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t x = i < n ? off[i] : 0u;
        uint32_t incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d);
            if ((int)lane >= d) incl += y;
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16u; w++) {
            before += w < wave ? wave_sum[w] : 0u;
            total += wave_sum[w];
        }
        if (i < n) off[i] = carry + before + incl - x;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0u) off[n] = carry;
}

// eid[], esrc[], eent[]: a wavefront per row
__global__ __launch_bounds__(256) void truss_number_kernel(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ row_idx,
                                                           uint32_t n, uint32_t nz_base, const uint32_t *__restrict__ off,
                                                           uint32_t *__restrict__ eid, uint32_t *__restrict__ esrc, uint32_t *__restrict__ eent) {
    const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * 4u;
    for (uint64_t v = blockIdx.x * 4u + (threadIdx.x >> 6); v < n; v += nwaves) {
        const uint32_t b = row_ptr[v] - nz_base, len = row_ptr[v + 1u] - nz_base - b;
        const uint32_t first = off[v], upper_at = len - (off[v + 1u] - first);
        for (uint32_t i = lane; i < len; i += 64u) {
            const uint32_t u = row_idx[b + i];
            uint32_t e = kTrNone;
            if (u > (uint32_t)v) {
                e = first + (i - upper_at);
                esrc[e] = (uint32_t)v;
                eent[e] = b + i;
            } else if (u < (uint32_t)v) {                            // the mirror entry: its partner (u, v) sits above u's diagonal
                const uint32_t bu = row_ptr[u] - nz_base, lenu = row_ptr[u + 1u] - nz_base - bu;
                const uint32_t at = rows_lower_bound(row_idx + bu, lenu, (uint32_t)v);
                e = off[u] + (at - (lenu - (off[u + 1u] - off[u])));
            }
            eid[b + i] = e;
        }
    }
}

__global__ void truss_init_kernel(uint32_t *ctl) {
    if (blockIdx.x == 0u && threadIdx.x < 64u) ctl[threadIdx.x] = threadIdx.x == kTrussNext ? kTrNone : 0u;   // l = 0, phase scan, tail 0
}

// the two rows of edge e, the shorter first: (owner, begin, length) each
struct TrPair {
    uint32_t a, ab, alen, b, bb, blen;
};
__device__ __forceinline__ TrPair tr_pair(const TrArgs &a, uint32_t e) {
    const uint32_t u = a.esrc[e], v = a.row_idx[a.eent[e]];
    const uint32_t ub = a.row_ptr[u] - a.nz_base, ulen = a.row_ptr[u + 1u] - a.nz_base - ub;
    const uint32_t vb = a.row_ptr[v] - a.nz_base, vlen = a.row_ptr[v + 1u] - a.nz_base - vb;
    if (ulen <= vlen) return {u, ub, ulen, v, vb, vlen};
    return {v, vb, vlen, u, ub, ulen};
}

// S[e] = |N(u) & N(v)| for every edge, and the sum of them all: 64 >> g_shift edges per wavefront
__global__ __launch_bounds__(256) void truss_support_kernel(TrArgs a) {
    const uint32_t lane = threadIdx.x & 63u, group = 1u << a.g_shift, sub = lane & (group - 1u), per = 64u >> a.g_shift;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4u;
    unsigned long long sum = 0;
    for (uint64_t base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (uint64_t)per; base < a.m; base += nwaves * per) {
        const uint64_t e = base + (lane >> a.g_shift);
        uint32_t count = 0;
        if (e < a.m) {
            const TrPair r = tr_pair(a, (uint32_t)e);
            for (uint32_t i = sub; i < r.alen; i += group) {
                const uint32_t w = a.row_idx[r.ab + i];
                if (w == r.a || w == r.b) continue;
                count += a.row_idx[r.bb + rows_lower_bound(a.row_idx + r.bb, r.blen, w)] == w ? 1u : 0u;
            }
        }
        uint32_t of_group = 0;                                       // (every lane takes every step of the butterfly)
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            if (d == group) of_group = count;
            count += (uint32_t)__shfl_xor(count, (int)d);
        }
        if (group == 64u) of_group = count;
        if (sub == 0u && e < a.m) a.S[e] = of_group;
        sum += count;
    }
    if (lane == 0u && sum != 0ull) ga_add((unsigned long long *)(a.ctl + kTrussSum), sum);
}

__global__ __launch_bounds__(256) void truss_scan_kernel(TrArgs a) {
    if (a.ctl[kPeelPhase] != kPeelScan) return;
    const uint32_t l = a.ctl[kPeelLevel], lane = threadIdx.x & 63u;
    const uint64_t mround = ((uint64_t)a.m + 255u) & ~255ull;     // whole wavefronts take every trip
    uint32_t next = kTrNone;
    for (uint64_t e = blockIdx.x * 256u + threadIdx.x; e < mround; e += gridDim.x * 256u) {
        const bool open = e < a.m && a.pos[e] == kTrNone;
        const uint32_t s = open ? a.S[e] : 0u;
        const bool hit = open && s == l;
        if (open && s > l) next = min(next, s);
        const uint32_t at = wave_append(hit, a.ctl + kPeelTail, lane);
        if (hit && at < a.m) {                                       // (at < m: every edge is appended once)
            a.queue[at] = (uint32_t)e;
            a.pos[e] = at;
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) next = min(next, (uint32_t)__shfl_xor(next, d));
    if (lane == 0u && next != kTrNone) ga_min(a.ctl + kTrussNext, next);
}

// one triangle less for edge x, at level l
__device__ __forceinline__ void tr_decrement(const TrArgs &a, uint32_t x, uint32_t l) {
    uint32_t old = ga_load(a.S + x);
    while (old > l) {
        const uint32_t less = old - 1u;
        if (ga_cas(a.S + x, old, less)) {
            if (less == l) {
                const uint32_t at = ga_add(a.ctl + kPeelTail, 1u);
                if (at < a.m) {
                    a.queue[at] = x;
                    ga_store(a.pos + x, at);
                }
            }
            return;
        }
    }
}

__global__ __launch_bounds__(256) void truss_peel_kernel(TrArgs a) {
    if (a.ctl[kPeelPhase] != kPeelPeel) return;
    const uint32_t l = a.ctl[kPeelLevel], lo = a.ctl[kPeelLo], hi = a.ctl[kPeelHi];
    // lanes per edge: truss_group, and more while the slice leaves half the launch idle (late sub-rounds hold a few hub edges whose
    // rows one group would walk alone) -- up to 1 << truss_spread lanes, across wavefronts and workgroups: nothing is reduced here
    const uint64_t threads = (uint64_t)gridDim.x * 256u, me = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t shift = a.g_shift;
    while (shift < a.spread_shift && ((uint64_t)(hi - lo) << (shift + 1u)) <= threads) shift++;
    const uint32_t group = 1u << shift, sub = (uint32_t)me & (group - 1u);
    const uint64_t ngroups = threads >> shift;
    for (uint64_t item = me >> shift; item < hi - lo; item += ngroups) {
        const uint32_t e = a.queue[lo + item];
        const TrPair r = tr_pair(a, e);
        for (uint32_t i = sub; i < r.alen; i += group) {
            const uint32_t w = a.row_idx[r.ab + i];
            if (w == r.a || w == r.b) continue;
            const uint32_t at = rows_lower_bound(a.row_idx + r.bb, r.blen, w);
            if (a.row_idx[r.bb + at] != w) continue;
            const uint32_t e1 = a.eid[r.ab + i], e2 = a.eid[r.bb + at];
            const uint32_t p1 = ga_load(a.pos + e1), p2 = ga_load(a.pos + e2);
            if (p1 < lo || p2 < lo) continue;
            const bool in1 = p1 < hi, in2 = p2 < hi;
            if (in1 && in2) continue;
            if (in1) {
                if (e < e1) tr_decrement(a, e2, l);
            } else if (in2) {
                if (e < e2) tr_decrement(a, e1, l);
            } else {
                tr_decrement(a, e1, l);
                tr_decrement(a, e2, l);
            }
        }
    }
}

// behind exactly one scan or peel that ran (plain loads and stores: a launch of its own)
__global__ void truss_turn_kernel(uint32_t *ctl, uint32_t m) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    const uint32_t phase = ctl[kPeelPhase];
    if (phase == kPeelDone) return;
    const uint32_t l = ctl[kPeelLevel], lo = ctl[kPeelHi], hi = min(ctl[kPeelTail], m), next = ctl[kTrussNext];
    ctl[kPeelLo] = lo;
    ctl[kPeelHi] = hi;
    ctl[kTrussNext] = kTrNone;
    if (hi != lo) ctl[kPeelSubRounds] += 1u;
    const bool done = hi >= m, over = lo == hi;
    if ((done || over) && hi != ctl[kPeelLevelStart]) {             // the level queued somebody: its edges have truss l + 2
        ctl[kPeelLevels] += 1u;
        ctl[kPeelLevelStart] = hi;
        ctl[kPeelTop] = l;
    }
    if (done) {
        ctl[kPeelPhase] = kPeelDone;
    } else if (over) {
        // a scan that queued nobody saw every open edge, and nothing was decremented since: jump to the smallest word it saw
        ctl[kPeelLevel] = phase == kPeelScan && next != kTrNone ? next : l + 1u;
        ctl[kPeelPhase] = kPeelScan;
    } else {
        ctl[kPeelPhase] = kPeelPeel;
    }
}

// out[j] = S[eid[j]] + add for every entry, 0 on the diagonal; with `gate` (the control record) only once the phase is "done"
__global__ __launch_bounds__(256) void truss_write_kernel(const uint32_t *__restrict__ eid, const uint32_t *__restrict__ S, uint64_t nnz,
                                                          uint32_t add, uint32_t *__restrict__ out, const uint32_t *gate) {
    if (gate && gate[kPeelPhase] != kPeelDone) return;
    for (uint64_t j = blockIdx.x * 256u + threadIdx.x; j < nnz; j += gridDim.x * 256u) {
        const uint32_t e = eid[j];
        out[j] = e == kTrNone ? 0u : S[e] + add;
    }
}

// the words of the plan's scratch: the control record, off[n + 1], eid[nnz], then five arrays of nnz / 2 >= m words
struct TrLayout {
    uint32_t *ctl, *off, *eid, *esrc, *eent, *S, *queue, *pos;
    size_t bytes;
};
static TrLayout truss_layout(gl_spmv_plan p) {
    const size_t n = p->num_rows, nnz = (size_t)p->nnz, cap = nnz / 2u;
    TrLayout t;
    t.ctl = reinterpret_cast<uint32_t *>(p->d_truss_scratch);
    t.off = t.ctl + kRoundsCtlBytes / 4u;
    t.eid = t.off + n + 1u;
    t.esrc = t.eid + nnz;
    t.eent = t.esrc + cap;
    t.S = t.eent + cap;
    t.queue = t.S + cap;
    t.pos = t.queue + cap;
    t.bytes = kRoundsCtlBytes + 4u * (n + 1u + nnz + 5u * cap);
    return t;
}

// the refusals, the plan's verdicts, its scratch and its edge numbering, on first use
static int truss_prepare(gl_spmv_plan p, const char *who) {
    int rc = rows_require(p, kRowsSymmetric, who, "the plan", "io.symmetrize_simple");
    if (rc != GL_OK || p->nnz == 0 || p->truss_edges >= 0) return rc;
    rc = plan_scratch(p->d_truss_scratch, truss_layout(p).bytes, who, "control record, edge numbering, supports, queue and positions");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const TrLayout t = truss_layout(p);
    const uint32_t n = p->num_rows;
    truss_upper_kernel<<<rows_stream_grid(n), 256, 0, s>>>(p->d_csr_indptr, p->d_csr_indices, n, p->csr_nz_base, t.off);
    truss_offsets_kernel<<<1, 1024, 0, s>>>(t.off, n);
    truss_number_kernel<<<std::max(1u, std::min<unsigned>(cdiv(n, 4u), (unsigned)ctx().num_cus * 8u)), 256, 0, s>>>(
        p->d_csr_indptr, p->d_csr_indices, n, p->csr_nz_base, t.off, t.eid, t.esrc, t.eent);
    GL_LAUNCH_CHECK();
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    GL_HIP(hipMemcpyAsync(w, t.off + n, 4u, hipMemcpyDeviceToHost, s));
    GL_HIP(hipStreamSynchronize(s));
    if ((uint64_t)w[0] > p->nnz / 2u)
        return set_error(GL_ERR_HIP, "%s: internal error: %u edges numbered among %llu entries", who, w[0], (unsigned long long)p->nnz);
    p->truss_edges = (int64_t)w[0];
    return GL_OK;
}

static int truss(gl_spmv_plan p, uint32_t *d_truss, uint32_t *d_support, uint64_t *h_stats, const char *who) {
    int rc = truss_prepare(p, who);
    if (rc != GL_OK) return rc;
    if (h_stats) std::fill(h_stats, h_stats + 6, 0ull);
    if (p->num_rows == 0u || p->nnz == 0) return GL_OK;           // no entries: nothing to write
    hipStream_t s = ctx().stream;
    const uint32_t m = (uint32_t)p->truss_edges;
    const uint64_t nnz = p->nnz;
    if (m == 0u) {                                                // only diagonal entries
        GL_HIP(hipMemsetAsync(d_truss, 0, 4u * (size_t)nnz, s));
        if (d_support) GL_HIP(hipMemsetAsync(d_support, 0, 4u * (size_t)nnz, s));
        return GL_OK;
    }
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 18): truss_group = lanes per edge in the support pass and
    // the peel (a power of two, 1 .. 64), truss_batch = (scan, peel, turn) triples enqueued between two read-backs of the control
    // record, truss_grid = workgroups per compute unit of a support or peel launch, truss_spread = log2 of the most lanes a peel
    // launch gives an edge when its slice is short (0: never more than truss_group).  Defaults: 64 (the best of 1 .. 64 on the
    // call and on the support pass), 64 (1 is 33 - 51 % slower, 16 and 256 within 4 %), 8 (2 and 4 are slower on the support pass,
    // 16 equals 8) and 10 (0 and 6: 1.8 times slower -- 4.5 times at truss_group 16 --, 8 / 12 / 14: 4 - 12 % slower).  truss_support_only = 1 is a MEASUREMENT hook
    // (benchmarks/bench_truss.py times the support pass with it): the call ends behind the support pass, d_truss then holds
    // support + 2 -- an upper bound, not the truss number -- and the stats carry only launches, edges and triangles
    const long want_group = std::max<long>(1, std::min<long>(debug_knob("truss_group", 64), 64));
    const uint32_t batch = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("truss_batch", 64), 4096));
    const unsigned per_cu = (unsigned)std::max<long>(1, std::min<long>(debug_knob("truss_grid", 8), 1024));
    const long spread = std::max<long>(0, std::min<long>(debug_knob("truss_spread", 10), 16));
    const TrLayout t = truss_layout(p);
    TrArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.eid = t.eid;
    a.esrc = t.esrc;
    a.eent = t.eent;
    a.S = t.S;
    a.queue = t.queue;
    a.pos = t.pos;
    a.ctl = t.ctl;
    a.m = m;
    a.nz_base = p->csr_nz_base;
    a.g_shift = 0;
    while ((2l << a.g_shift) <= want_group) a.g_shift++;          // (rounded down to a power of two)
    a.spread_shift = std::max<uint32_t>(a.g_shift, (uint32_t)spread);
    const unsigned cap_grid = (unsigned)ctx().num_cus * per_cu;
    const unsigned edge_grid = std::max(1u, std::min<unsigned>(cdiv(m, 256u), (unsigned)ctx().num_cus * 8u));
    const unsigned group_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((((uint64_t)m << a.g_shift) + 255u) / 256u, cap_grid));
    const unsigned entry_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nnz + 255u) / 256u, (uint64_t)ctx().num_cus * 8u));
    uint32_t *w = nullptr;
    GL_HIP(staging_words(&w));
    static_assert(kTrussRecordWords <= 12u, "the record and the 64-bit sum fit the page-locked staging words");
    truss_init_kernel<<<1, 64, 0, s>>>(t.ctl);
    GL_HIP(hipMemsetAsync(t.pos, 0xff, 4u * (size_t)m, s));
    truss_support_kernel<<<group_grid, 256, 0, s>>>(a);
    if (d_support) truss_write_kernel<<<entry_grid, 256, 0, s>>>(t.eid, t.S, nnz, 0u, d_support, nullptr);
    GL_LAUNCH_CHECK();
    uint64_t launches = d_support ? 3 : 2;
    if (debug_knob("truss_support_only", 0) != 0) {
        truss_write_kernel<<<entry_grid, 256, 0, s>>>(t.eid, t.S, nnz, 2u, d_truss, nullptr);
        GL_LAUNCH_CHECK();
        GL_HIP(hipMemcpyAsync(w + 12, t.ctl + kTrussSum, 8u, hipMemcpyDeviceToHost, s));
        GL_HIP(hipStreamSynchronize(s));
        if (h_stats) {
            uint64_t sum;
            std::memcpy(&sum, w + 12, 8);
            h_stats[3] = launches + 1;
            h_stats[4] = m;
            h_stats[5] = sum / 3u;
        }
        return GL_OK;
    }
    // every step that runs is a scan (one per level looked at: at most max support + 1 <= m of them) or a sub-round over a slice
    // that is not empty (every edge is in one slice): at most 2 m + 1 steps
    rc = rounds_run(
        batch, 2ull * m + 1ull, launches,
        [&] {
            for (uint32_t i = 0; i < batch; i++) {
                truss_scan_kernel<<<edge_grid, 256, 0, s>>>(a);
                truss_peel_kernel<<<group_grid, 256, 0, s>>>(a);
                truss_turn_kernel<<<1, 64, 0, s>>>(t.ctl, m);
            }
            truss_write_kernel<<<entry_grid, 256, 0, s>>>(t.eid, t.S, nnz, 2u, d_truss, t.ctl);   // (runs in the batch that ends the peel)
            return 3ull * batch + 1ull;
        },
        [&] {
            const hipError_t e = hipMemcpyAsync(w, t.ctl, kTrussRecordWords * 4u, hipMemcpyDeviceToHost, s);
            return e != hipSuccess ? e : hipMemcpyAsync(w + 12, t.ctl + kTrussSum, 8u, hipMemcpyDeviceToHost, s);
        },
        [&] { return w[kPeelPhase] == kPeelDone ? kRoundsDone : kRoundsGoOn; },
        [&](uint64_t steps) {
            return set_error(GL_ERR_HIP, "%s: internal error: not done after %llu steps on %u edges (level %u, slice [%u, %u), %u sub-rounds)",
                             who, (unsigned long long)steps, m, w[kPeelLevel], w[kPeelLo], w[kPeelHi], w[kPeelSubRounds]);
        });
    if (rc != GL_OK) return rc;
    if (h_stats) {
        uint64_t sum;
        std::memcpy(&sum, w + 12, 8);
        h_stats[0] = (uint64_t)w[kPeelTop] + 2u;
        h_stats[1] = w[kPeelLevels];
        h_stats[2] = w[kPeelSubRounds];
        h_stats[3] = launches;
        h_stats[4] = m;
        h_stats[5] = sum / 3u;
    }
    return GL_OK;
}

}  // namespace gl

int gl_truss(gl_spmv_plan plan, uint32_t *d_truss, uint32_t *d_support, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_truss != nullptr);
    GL_ARG(d_support != d_truss);
    return gl::truss(plan, d_truss, d_support, h_stats, "gl_truss");
}
