// Neighbourhood similarity (gl_similarity): the common neighbours of CALLER-CHOSEN pairs of vertices over the plain CSR copy that a
// GL_PLAN_BOOLEAN plan keeps (gl_spmv_plan.h: d_csr_indptr / d_csr_indices / csr_nz_base), on a square, whole-matrix plan whose rows
// are strictly ascending sets N(x) (gl_rows.h: kRowsSets).  With n = num_rows, for the pair i = (u, v):
//
//   common[i]   = |N(u) & N(v)|                                                               (u32)
//   weighted[i] = the sum of weight[w] over the w of N(u) & N(v), modulo 2^64                 (u64, optional)
//
// u >= n or v >= n: common = 0xffffffff, weighted = 0, and the pair is counted.  The weights are INTEGERS on purpose: integer adds
// commute, so the lanes' registers, the shuffle tree and any group width give the same bits, and there is no floating-point
// operation in this file.  gl_tc and gl_truss intersect rows too, but only of pairs that are entries; here the pairs need not be.
//
// TWO PASSES per chunk of at most 2^20 pairs, enqueued in stream order without a host synchronisation between:
//   short  a sub-wave GROUP of G lanes (sim_group: 8, 16, 32, 64) per pair, 256 / G pairs per workgroup.  The group orders the two
//          rows by length -- degrees come from the row offsets --, WALKS the shorter, G entries per step (coalesced), and every
//          lane looks its entry up in the LONGER by rows_lower_bound in global memory (the first probes of all lanes coincide): the
//          form gl_tc's tc_search=1 takes.  Hits and weights are summed per lane in registers, then over the group's lanes by
//          shuffles; the group's lane 0 stores the two words.  A pair whose shorter row has more than sim_short entries is DEFERRED:
//          its index in the chunk is appended to the list (gl_rounds.h: wave_append; the order does not matter, the outputs are per
//          pair) and nothing is stored for it.
//   long   a wavefront per listed pair, the same loop at G = 64, grid-striding over the list, whose length it reads from the
//          control record.
// Every output word has ONE writer, its pair's group; no atomic touches an output.  Groups share no LDS (the kernels use none) and
// meet at no barrier.  No spin-waits, no hand-offs between workgroups.  The kernels read offsets, columns, pairs and weights only.
// MEMORY RULE (gl_rounds.h): atomic-only inside a launch are the control words of the second line -- the two list tails, which
// the chunks take in turn (the long pass of a chunk zeroes the tail of the next one: nobody else touches that word in its
// launch), the count of pairs out of range and the count of deferred pairs.  The list's entries are plain words, written by the
// short pass and read by the long pass behind a launch boundary.
#include "gl_rounds.h"
#include "graphlily_hip_sim.h"

namespace gl {

enum : uint32_t { kSimTail = 32, kSimOutOfRange = 34, kSimDeferred = 35 };      // (kSimTail + the chunk's parity)
constexpr uint32_t kSimChunk = 1u << 20;                                        // pairs per chunk: the list's words
constexpr uint32_t kSimNone = 0xffffffffu;                                      // the count of a pair out of range
constexpr size_t kSimScratchBytes = kRoundsCtlBytes + 4u * (size_t)kSimChunk;

struct SimArgs {
    const uint32_t *row_ptr, *row_idx, *pairs;
    const unsigned long long *weight;
    uint32_t *common, *ctl, *list;
    unsigned long long *weighted;
    uint32_t n, nz_base, m, cap, parity;   // m: the pairs of this chunk, to which pairs, common and weighted point
};

// what the G lanes of a group (lane gl of it) find of the shorter row ns[0 .. ls) in the longer nl[0 .. ll), ls <= ll: per lane.
// The step is min(G, what is left), so no position is formed behind ls whatever the offsets.
template <int G, bool W>
__device__ __forceinline__ void sim_intersect(const uint32_t *__restrict__ ns, uint32_t ls, const uint32_t *__restrict__ nl, uint32_t ll,
                                              const unsigned long long *__restrict__ weight, uint32_t gl, uint32_t &hits,
                                              unsigned long long &sum) {
    for (uint32_t base = 0; base < ls; base += min((uint32_t)G, ls - base)) {
        if (ls - base > gl) {
            const uint32_t x = ns[base + gl];
            const bool hit = nl[rows_lower_bound(nl, ll, x)] == x;
            hits += hit ? 1u : 0u;
            if (W && hit) sum += weight[x];
        }
    }
}

// the pair's two rows, the shorter first (a tie keeps the order given: the intersection is the same)
struct SimRows {
    const uint32_t *ns, *nl;
    uint32_t ls, ll;
};
__device__ __forceinline__ SimRows sim_rows(const SimArgs &a, uint32_t u, uint32_t v) {
    const uint32_t ub = a.row_ptr[u], lu = a.row_ptr[u + 1u] - ub, vb = a.row_ptr[v], lv = a.row_ptr[v + 1u] - vb;
    const bool swap = lv < lu;
    SimRows r;
    r.ns = a.row_idx + ((swap ? vb : ub) - a.nz_base);
    r.nl = a.row_idx + ((swap ? ub : vb) - a.nz_base);
    r.ls = swap ? lv : lu;
    r.ll = swap ? lu : lv;
    return r;
}

template <int G, bool W>
__global__ __launch_bounds__(256) void sim_short_kernel(SimArgs a) {
    constexpr uint32_t kGroups = 256u / G;
    const uint32_t gl = threadIdx.x & (G - 1u), grp = threadIdx.x / G, lane = threadIdx.x & 63u;
    uint32_t bad = 0;                                             // pairs out of range this wavefront met (counted by lane gl == 0)
    // (base is the same in every lane of the workgroup: every lane takes every step, as wave_append asks)
    for (uint64_t base = (uint64_t)blockIdx.x * kGroups; base < a.m; base += (uint64_t)gridDim.x * kGroups) {
        const uint64_t i64 = base + grp;
        const bool in = i64 < a.m;
        const uint32_t i = (uint32_t)i64;
        uint32_t u = 0, v = 0;
        if (in) {
            u = a.pairs[2ull * i];
            v = a.pairs[2ull * i + 1ull];
        }
        const bool ok = in && u < a.n && v < a.n;
        SimRows r = {nullptr, nullptr, 0u, 0u};
        if (ok) r = sim_rows(a, u, v);
        const bool defer = r.ls > a.cap;
        const uint32_t at = wave_append(defer && gl == 0u, a.ctl + kSimTail + a.parity, lane);
        if (defer && gl == 0u) a.list[at] = i;                    // at < m <= kSimChunk: a pair is appended once
        uint32_t hits = 0;
        unsigned long long sum = 0ull;
        sim_intersect<G, W>(r.ns, defer ? 0u : r.ls, r.nl, r.ll, a.weight, gl, hits, sum);
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {               // (all lanes of a group are here together)
            hits += __shfl_xor(hits, off);
            if (W) sum += __shfl_xor(sum, off);
        }
        if (in && !defer && gl == 0u) {
            a.common[i] = ok ? hits : kSimNone;
            if (W) a.weighted[i] = sum;
            bad += ok ? 0u : 1u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
    if (lane == 0u && bad != 0u) (void)ga_add(a.ctl + kSimOutOfRange, bad);
}

template <bool W>
__global__ __launch_bounds__(256) void sim_long_kernel(SimArgs a) {
    const uint32_t count = min(a.ctl[kSimTail + a.parity], a.m);  // written by the short pass, a launch ago
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + wave; it < count; it += (uint64_t)gridDim.x * 4u) {
        const uint32_t i = a.list[it];                            // < m, in range, the shorter row not empty: the short pass saw to it
        const SimRows r = sim_rows(a, a.pairs[2ull * i], a.pairs[2ull * i + 1ull]);
        uint32_t hits = 0;
        unsigned long long sum = 0ull;
        sim_intersect<64, W>(r.ns, r.ls, r.nl, r.ll, a.weight, lane, hits, sum);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            hits += __shfl_xor(hits, off);
            if (W) sum += __shfl_xor(sum, off);
        }
        if (lane == 0u) {
            a.common[i] = hits;
            if (W) a.weighted[i] = sum;
        }
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        if (count != 0u) (void)ga_add(a.ctl + kSimDeferred, count);
        ga_store(a.ctl + kSimTail + (a.parity ^ 1u), 0u);         // the next chunk's tail: its short pass is the next launch
    }
}

// a plan without entries: every row is empty
__global__ __launch_bounds__(256) void sim_empty_kernel(SimArgs a) {
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.m; i += (uint64_t)gridDim.x * 256u) {
        const bool ok = a.pairs[2ull * i] < a.n && a.pairs[2ull * i + 1ull] < a.n;
        a.common[i] = ok ? 0u : kSimNone;
        if (a.weighted) a.weighted[i] = 0ull;
        bad += ok ? 0u : 1u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
    if ((threadIdx.x & 63u) == 0u && bad != 0u) (void)ga_add(a.ctl + kSimOutOfRange, bad);
}

template <int G>
static void sim_launch_short(const SimArgs &a, bool weighted, unsigned grid, hipStream_t s) {
    if (weighted) sim_short_kernel<G, true><<<grid, 256, 0, s>>>(a);
    else sim_short_kernel<G, false><<<grid, 256, 0, s>>>(a);
}

static int similarity(gl_spmv_plan p, const uint32_t *d_pairs, uint64_t m, const uint64_t *d_vertex_weight, uint32_t *d_common,
                      uint64_t *d_weighted, uint64_t *h_stats, const char *who) {
    int rc = rows_require(p, kRowsSets, who, "the plan", "io.symmetrize_simple (io.simple_pattern for a directed pattern)");
    if (rc != GL_OK) return rc;
    if (m > 0xffffffffull) return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: %llu pairs, at most 2^32 - 1", who, (unsigned long long)m);
    if (d_weighted && !d_vertex_weight)
        return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: d_weighted without d_vertex_weight", who);
    if (m != 0 && (!d_pairs || !d_common)) return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: a NULL d_pairs or d_common with m > 0", who);
    {
        const char *x[3] = {(const char *)d_pairs, (const char *)d_common, (const char *)d_weighted};
        const size_t bytes[3] = {8u * (size_t)m, 4u * (size_t)m, 8u * (size_t)m};
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; x[i] && j < 3; j++)
                if (x[j] && x[i] < x[j] + bytes[j] && x[j] < x[i] + bytes[i])
                    return set_error(GL_ERR_INVALID_ARG, "%s: invalid argument: the outputs overlap each other or the pairs", who);
    }
    if (h_stats) h_stats[0] = h_stats[1] = h_stats[2] = h_stats[3] = 0u;
    if (m == 0) return GL_OK;
    // A/B knobs (GRAPHLILY_DEBUG, read per call; EXPERIMENTS.md Round 30): sim_group = lanes per short pair (8, 16, 32 or 64),
    // sim_short = the longest shorter row the short pass answers (0 defers every pair whose shorter row is not empty), sim_grid =
    // workgroups per compute unit; sim_chunk (for the tests: the chunk boundary at a small m) = pairs per chunk
    const long group = debug_knob("sim_group", 16);
    const uint32_t cap = (uint32_t)std::max<long>(0, std::min<long>(debug_knob("sim_short", 64), 0x7fffffffl));
    const unsigned most = (unsigned)ctx().num_cus * (unsigned)std::max<long>(1, std::min<long>(debug_knob("sim_grid", 16), 1024));
    const uint32_t chunk = (uint32_t)std::max<long>(1, std::min<long>(debug_knob("sim_chunk", kSimChunk), kSimChunk));
    rc = plan_scratch(p->d_sim_scratch, kSimScratchBytes, who, "control record and the list of deferred pairs");
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const bool weighted = d_weighted != nullptr;
    SimArgs a;
    a.row_ptr = p->d_csr_indptr;
    a.row_idx = p->d_csr_indices;
    a.nz_base = p->csr_nz_base;
    a.weight = reinterpret_cast<const unsigned long long *>(d_vertex_weight);
    a.ctl = reinterpret_cast<uint32_t *>(p->d_sim_scratch);
    a.list = reinterpret_cast<uint32_t *>(p->d_sim_scratch + kRoundsCtlBytes);
    a.n = p->num_rows;
    a.cap = cap;
    GL_HIP(hipMemsetAsync(a.ctl, 0, kRoundsCtlBytes, s));
    uint64_t launches = 0;
    for (uint64_t base = 0, c = 0; base < m; base += chunk, c++) {
        a.m = (uint32_t)std::min<uint64_t>(chunk, m - base);
        a.pairs = d_pairs + 2u * base;
        a.common = d_common + base;
        a.weighted = weighted ? reinterpret_cast<unsigned long long *>(d_weighted) + base : nullptr;
        a.parity = (uint32_t)(c & 1u);
        if (p->nnz == 0) {
            sim_empty_kernel<<<std::max(1u, std::min(cdiv(a.m, 256u), most)), 256, 0, s>>>(a);
            launches += 1;
        } else {
            switch (group) {
                case 8: sim_launch_short<8>(a, weighted, std::max(1u, std::min(cdiv(a.m, 32u), most)), s); break;
                case 32: sim_launch_short<32>(a, weighted, std::max(1u, std::min(cdiv(a.m, 8u), most)), s); break;
                case 64: sim_launch_short<64>(a, weighted, std::max(1u, std::min(cdiv(a.m, 4u), most)), s); break;
                default: sim_launch_short<16>(a, weighted, std::max(1u, std::min(cdiv(a.m, 16u), most)), s); break;
            }
            const unsigned grid = std::max(1u, std::min(cdiv(a.m, 4u), most));
            if (weighted) sim_long_kernel<true><<<grid, 256, 0, s>>>(a);
            else sim_long_kernel<false><<<grid, 256, 0, s>>>(a);
            launches += 2;
        }
        GL_LAUNCH_CHECK();
    }
    if (h_stats) {
        uint32_t *w = nullptr;
        GL_HIP(staging_words(&w));
        GL_HIP(hipMemcpyAsync(w, a.ctl + kSimOutOfRange, 8u, hipMemcpyDeviceToHost, s));
        GL_HIP(hipStreamSynchronize(s));
        h_stats[0] = w[0];
        h_stats[1] = w[1];
        h_stats[2] = launches;
    }
    return GL_OK;
}

}  // namespace gl

int gl_similarity(gl_spmv_plan plan, const uint32_t *d_pairs, uint64_t m, const uint64_t *d_vertex_weight, uint32_t *d_common,
                  uint64_t *d_weighted, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr);
    return gl::similarity(plan, d_pairs, m, d_vertex_weight, d_common, d_weighted, h_stats, "gl_similarity");
}
