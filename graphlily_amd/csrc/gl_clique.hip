// k-clique counting (gl_clique_count, graphlily_hip_clique.h): AND + popcount on bit matrices, over the plain CSR copy that every
// GL_PLAN_BOOLEAN plan keeps, on a square, whole-matrix plan whose rows are strictly ascending sets N+(v) -- gl_tc_count's contract.
//
//   total  = number of sequences (v1, ..., vk) with vj in N+(vi) for every i < j                      (64 bits, wrapping)
//   per[x] = number of positions that x holds in those sequences                                       (64 bits each, optional)
//
// A formula about sets, as gl_tc_count's is (and for k = 3 the same one, to the bit): an acyclic orientation (io.orient_by_rank)
// gives every k-clique once, a full symmetric pattern k! times, a diagonal entry simply takes part.  Integer adds commute, so
// the result is exact whatever the schedule.
//
// THE WORK FOR A SOURCE v with d = |N+(v)| >= k - 1 is c_{k-1} of the subgraph induced on its row (kClist), in three steps:
//   stage   N+(v) goes to LDS as the sorted list L[0 .. d)
//   build   the local bit matrix B, d rows of W = ceil(d / 32) words: bit j of B[i] is set iff L[j] is in N+(L[i]).  For every i
//           N+(L[i]) is loaded in coalesced pieces, every lane looks its w up in L (rows_lower_bound: gl_tc_count's two-hop
//           stream) and a hit sets its bit with an atomic OR
//   count   on bitsets only, the row lists are not touched again.  A group of G lanes holds one candidate set, word gl + G q in
//           lane gl, in registers, one set per depth (the recursion is a template: the stack of k - 3 sets is registers).  A
//           work item is a first-level local vertex i with the root set B[i]; descending to member l of a set S is one read of
//           B[l]'s word per lane and one AND, and at the last level a popcount.  The next member of S comes from a ballot of the
//           non-zero words, ffs and a read-lane.  k = 3 is the popcount of B, k = 4 the sum over (i, j in B[i]) of
//           popc(B[i] & B[j]).
// Zeroing, building and counting are separated by a workgroup barrier (a wavefront fence where one wavefront owns the matrix).
// No spin-waits, no hand-offs between workgroups, no floating point.
//
// THE PLAN'S FIRST CALL has it established that the rows are such sets (gl_rows.h: kRowsSets), reads the row offsets back once
// and bins the rows that can hold a sequence (two entries and more; one where the plan has a diagonal entry, which one launch
// finds out) by d, longest first inside a bin; bins, caps and the slabs are cached in the plan:
//   tiny   d <= clique_tiny (32)     a group of 32 lanes per vertex, B is 32 words in the group's LDS slice, a LANE per first-level
//                                    vertex runs a private depth-first loop on 32-bit masks
//   mid    d <= clique_mid (256)     a workgroup of four wavefronts per vertex shares the matrix (<= 8 KiB), G = 8
//   wide   d <= clique_lds (1024)    a workgroup of sixteen wavefronts per vertex, the matrix up to 128 KiB of LDS plus L (the launch
//                                    asks for the bin's LONGEST row, not the cap; above 64 KiB by hipFuncSetAttribute), G = 32
//   long   d <= 8192                 the SAME template with the matrix in a global scratch slab per resident workgroup, G = 64 with
//                                    four words per lane; the grid is capped so that the slabs stay inside clique_scratch_mb (1024)
// clique_lds is the LDS budget: no row longer than it is staged in LDS, so clique_lds=0 sends every row to the slabs and
// clique_tiny=0 clique_mid=0 every row to the wide bin.  The caps are starting values.
//
// PER-VERTEX COUNTS are a template parameter (the total-only kernels carry none of it).  At a leaf with set S and prefix
// (v, i, j, ...) every member of S is credited 1 -- gathered over the leaves of one parent set in vertical counters, so that a
// member's credits leave as one add per 63 leaves -- and every prefix vertex popc(S), added on the way back up.  Credits go to 64-bit
// LDS words next to L (LDS atomics; the long bin adds to global memory directly) and reach per[] once per row, one 64-bit add
// per entry that earned any; per[v] is one add per row.  The total is one 64-bit atomic per wavefront at the end.
#include "gl_rows.h"
#include "graphlily_hip_clique.h"

namespace gl {

constexpr uint32_t kCliqueMaxTiny = 32, kCliqueMaxMid = 256, kCliqueMaxLds = 1024, kCliqueMaxRow = 8192;
constexpr uint32_t kCliqueLdsOptIn = 64u * 1024u;   // what a launch gets without asking

struct CliqueArgs {
    const uint32_t *row_ptr, *row_idx;
    const uint32_t *items;                 // row numbers of the bin, longest first
    unsigned long long *total, *per;
    uint32_t *slab;                        // long bin: slab_words words of matrix per workgroup
    uint32_t nitems, nz_base;
    uint32_t cap;                          // entries of L the launch has room for: the bin's longest row, rounded up to 2
    uint32_t min_d;                        // shorter rows hold no sequence: k - 1, or 1 where the plan has a diagonal entry
    uint32_t slab_words;
    uint32_t build_only;                   // clique_build_only=1 (benchmarks): stop behind the matrix, count nothing
};

// lanes of one wavefront have written the slice / are about to overwrite it (gl_tc.hip: tc_slice_sync)
__device__ __forceinline__ void clique_slice_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void clique_total(unsigned long long mine, unsigned long long *total) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63u) == 0u && mine != 0ull) atomicAdd(total, mine);
}

// VERTICAL COUNTERS for the per-vertex credits of a set's members at the last level: plane[b] holds bit b of a count per bit
// position of one word of the set, adding a child's word of 0 / 1s is a ripple of six AND / XORs, and a member's count of up
// to 63 children leaves as ONE credit -- not one atomic per clique
constexpr int kCliquePlanes = 6;
__device__ __forceinline__ void clique_planes_add(uint32_t (&plane)[kCliquePlanes], uint32_t bits) {
#pragma unroll
    for (int b = 0; b < kCliquePlanes; b++) {
        const uint32_t carry = plane[b] & bits;
        plane[b] ^= bits;
        bits = carry;
    }
}
// credit(bit, count) for every bit position with a count, then the planes are zero again
template <typename Credit>
__device__ __forceinline__ void clique_planes_flush(uint32_t (&plane)[kCliquePlanes], Credit &&credit) {
    uint32_t any = 0;
#pragma unroll
    for (int b = 0; b < kCliquePlanes; b++) any |= plane[b];
    for (uint32_t r = any; r; r &= r - 1u) {
        const uint32_t bit = (uint32_t)__ffs((int)r) - 1u;
        uint32_t n = 0;
#pragma unroll
        for (int b = 0; b < kCliquePlanes; b++) n |= ((plane[b] >> bit) & 1u) << b;
        credit(bit, n);
    }
#pragma unroll
    for (int b = 0; b < kCliquePlanes; b++) plane[b] = 0u;
}

// ------------------------------------------------------------------------------------------------------------- the tiny bin
// D descents left below the set S (one 32-bit mask: d <= 32), private to a lane -> the leaves below S
template <int D, bool PER>
__device__ __forceinline__ unsigned long long clique_dfs(uint32_t S, const uint32_t *B, unsigned long long *credit) {
    if constexpr (D == 0) {
        if (PER)
            for (uint32_t r = S; r; r &= r - 1u) atomicAdd(credit + (__ffs((int)r) - 1), 1ull);
        return (unsigned long long)__popc(S);
    } else if constexpr (D == 1 && PER) {
        // the last level with its leaves: at most 32 children, so the planes never overflow
        uint32_t plane[kCliquePlanes] = {0u, 0u, 0u, 0u, 0u, 0u};
        unsigned long long sum = 0;
        for (uint32_t r = S; r; r &= r - 1u) {
            const uint32_t l = (uint32_t)__ffs((int)r) - 1u, T = S & B[l];
            if (T != 0u) atomicAdd(credit + l, (unsigned long long)__popc(T));
            sum += (unsigned long long)__popc(T);
            clique_planes_add(plane, T);
        }
        clique_planes_flush(plane, [&](uint32_t bit, uint32_t n) { atomicAdd(credit + bit, (unsigned long long)n); });
        return sum;
    } else {
        unsigned long long sum = 0;
        for (uint32_t r = S; r; r &= r - 1u) {
            const uint32_t l = (uint32_t)__ffs((int)r) - 1u;
            const unsigned long long c = clique_dfs<D - 1, PER>(S & B[l], B, credit);
            if (PER && c != 0ull) atomicAdd(credit + l, c);
            sum += c;
        }
        return sum;
    }
}

template <int K, bool PER>
__global__ __launch_bounds__(256) void clique_tiny_kernel(CliqueArgs a) {
    extern __shared__ unsigned long long clique_lds[];
    const uint32_t gl = threadIdx.x & 31u, grp = threadIdx.x >> 5, groups = blockDim.x >> 5;
    // the group's slice: with per-vertex counts 32 credit words, then L and B, 32 words each
    unsigned long long *credit = clique_lds + grp * (PER ? 64u : 32u);
    uint32_t *L = reinterpret_cast<uint32_t *>(credit + (PER ? 32u : 0u));
    uint32_t *B = L + 32;
    unsigned long long mine = 0;
    for (uint32_t it = blockIdx.x * groups + grp; it < a.nitems; it += gridDim.x * groups) {
        const uint32_t v = a.items[it];
        const uint32_t beg = a.row_ptr[v], d = a.row_ptr[v + 1u] - beg;      // d <= 32: the host binned by these very offsets
        if (d < a.min_d) continue;
        const uint32_t *nv = a.row_idx + (beg - a.nz_base);
        clique_slice_sync();
        if (gl < d) L[gl] = nv[gl];
        B[gl] = 0u;
        if (PER) credit[gl] = 0ull;
        clique_slice_sync();
        for (uint32_t i = 0; i < d; i++) {
            const uint32_t u = L[i];                                         // < num_rows: established by the plan's first call
            const uint32_t ub = a.row_ptr[u], lu = a.row_ptr[u + 1u] - ub;
            const uint32_t *nu = a.row_idx + (ub - a.nz_base);
            for (uint32_t k = gl; k - gl < lu; k += 32u) {
                if (k < lu) {
                    const uint32_t w = nu[k], at = rows_lower_bound(L, d, w);
                    if (L[at] == w) atomicOr(B + i, 1u << at);
                }
            }
        }
        clique_slice_sync();
        if (a.build_only) continue;
        const unsigned long long c = gl < d ? clique_dfs<K - 3, PER>(B[gl], B, credit) : 0ull;
        if (PER) {
            if (c != 0ull) atomicAdd(credit + gl, c);
            clique_slice_sync();
            unsigned long long row = c;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) row += __shfl_xor(row, off);
            if (gl < d) {
                const unsigned long long earned = credit[gl];
                if (earned != 0ull) atomicAdd(a.per + L[gl], earned);
            }
            if (gl == 0u && row != 0ull) atomicAdd(a.per + v, row);
        }
        mine += c;
    }
    clique_total(mine, a.total);
}

// ------------------------------------------------------------------------------------------- the mid, wide and long bins
// a word of the matrix: in a slab it was written by atomics of other wavefronts, which the vector cache does not see
template <bool SLAB>
__device__ __forceinline__ uint32_t clique_word(const uint32_t *p) {
    return SLAB ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}

// what a group of G lanes carries down the recursion
struct CliqueGroup {
    const uint32_t *B, *L;
    unsigned long long *credit;            // LDS credit words, or per[] in the long bin
    uint32_t W, gl, gbase;                 // words per matrix row; the lane in its group; the group's first lane in its wavefront
    unsigned long long mine;               // total-only: this lane's popcounts
};

template <bool SLAB>
__device__ __forceinline__ void clique_credit(const CliqueGroup &g, uint32_t local, unsigned long long n) {
    if (SLAB) atomicAdd(g.credit + g.L[local], n);
    else atomicAdd(g.credit + local, n);
}

// the next member of what is left of a set (word gl + G q of it in rem[q]): the first lane of the group with a non-zero word, the
// lowest bit of its first such word -- a ballot, ffs and a read-lane -> false when nothing is left; the member leaves rem
template <int G, int WPL>
__device__ __forceinline__ bool clique_next_member(uint32_t (&rem)[WPL], const CliqueGroup &g, uint32_t &l) {
    constexpr unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    uint32_t mine_q = 0, word = rem[0];
#pragma unroll
    for (int q = 1; q < WPL; q++) {
        const bool take = word == 0u && rem[q] != 0u;
        mine_q = take ? (uint32_t)q : mine_q;
        word = take ? rem[q] : word;
    }
    const unsigned long long bal = (__ballot(word != 0u) >> g.gbase) & gmask;
    if (bal == 0ull) return false;
    const uint32_t src = (uint32_t)__ffsll(bal) - 1u;
    const uint32_t cand = (g.gl + (uint32_t)G * mine_q) * 32u + (uint32_t)__ffs((int)word) - 1u;
    l = (uint32_t)__shfl((int)cand, (int)(g.gbase + src));
    if (g.gl == src) {
#pragma unroll
        for (int q = 0; q < WPL; q++) rem[q] &= (uint32_t)q == mine_q ? rem[q] - 1u : ~0u;
    }
    return true;
}

// T = S & B[l]: one read of B[l]'s word per lane and word, one AND
template <int G, int WPL, bool SLAB>
__device__ __forceinline__ void clique_child(const uint32_t (&S)[WPL], uint32_t l, const CliqueGroup &g, uint32_t (&T)[WPL]) {
#pragma unroll
    for (int t = 0; t < WPL; t++) {
        const uint32_t wi = g.gl + (uint32_t)(G * t);
        T[t] = wi < g.W ? S[t] & clique_word<SLAB>(g.B + l * g.W + wi) : 0u;
    }
}

template <int G, int WPL>
__device__ __forceinline__ uint32_t clique_popc(const uint32_t (&S)[WPL]) {
    uint32_t p = 0;
#pragma unroll
    for (int q = 0; q < WPL; q++) p += (uint32_t)__popc(S[q]);
    return p;
}
template <int G>
__device__ __forceinline__ uint32_t clique_group_sum(uint32_t p) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) p += __shfl_xor(p, off);
    return p;
}

// D descents left below the set S (word gl + G q of it in S[q]) -> with per-vertex counts the leaves below S, the same in every
// lane of the group; without them 0, and every lane has added the popcounts of its own words to g.mine
template <int D, int G, int WPL, bool PER, bool SLAB>
__device__ __forceinline__ unsigned long long clique_set(const uint32_t (&S)[WPL], CliqueGroup &g) {
    if constexpr (D == 0) {
        const uint32_t p = clique_popc<G, WPL>(S);
        if (!PER) {
            g.mine += p;
            return 0ull;
        }
#pragma unroll
        for (int q = 0; q < WPL; q++)
            for (uint32_t r = S[q]; r; r &= r - 1u) clique_credit<SLAB>(g, (g.gl + (uint32_t)(G * q)) * 32u + (uint32_t)__ffs((int)r) - 1u, 1ull);
        return clique_group_sum<G>(p);
    } else if constexpr (D == 1 && PER) {
        // the last level with its leaves: the members' credits gather in the vertical counters, which leave every 63 children
        uint32_t plane[WPL][kCliquePlanes], rem[WPL], T[WPL], l = 0, pending = 0;
#pragma unroll
        for (int q = 0; q < WPL; q++) {
            rem[q] = S[q];
#pragma unroll
            for (int b = 0; b < kCliquePlanes; b++) plane[q][b] = 0u;
        }
        auto flush = [&]() {
#pragma unroll
            for (int q = 0; q < WPL; q++)
                clique_planes_flush(plane[q], [&](uint32_t bit, uint32_t n) {
                    clique_credit<SLAB>(g, (g.gl + (uint32_t)(G * q)) * 32u + bit, (unsigned long long)n);
                });
            pending = 0;
        };
        unsigned long long sum = 0;
        while (clique_next_member<G, WPL>(rem, g, l)) {
            clique_child<G, WPL, SLAB>(S, l, g, T);
            const uint32_t c = clique_group_sum<G>(clique_popc<G, WPL>(T));
            if (g.gl == 0u && c != 0u) clique_credit<SLAB>(g, l, (unsigned long long)c);
            sum += c;
#pragma unroll
            for (int q = 0; q < WPL; q++) clique_planes_add(plane[q], T[q]);
            if (++pending == 63u) flush();
        }
        flush();
        return sum;
    } else {
        unsigned long long sum = 0;
        uint32_t rem[WPL], T[WPL], l = 0;
#pragma unroll
        for (int q = 0; q < WPL; q++) rem[q] = S[q];
        while (clique_next_member<G, WPL>(rem, g, l)) {
            clique_child<G, WPL, SLAB>(S, l, g, T);
            const unsigned long long c = clique_set<D - 1, G, WPL, PER, SLAB>(T, g);
            if (PER) {
                if (g.gl == 0u && c != 0ull) clique_credit<SLAB>(g, l, c);
                sum += c;
            }
        }
        return sum;
    }
}

template <int K, int G, int WPL, bool PER, bool SLAB>
__global__ __launch_bounds__(G == 8 ? 256 : 1024) void clique_kernel(CliqueArgs a) {
    extern __shared__ unsigned long long clique_lds[];
    const uint32_t tid = threadIdx.x, threads = blockDim.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6, waves = threads >> 6;
    const uint32_t grp = tid / G, groups = threads / G;
    // LDS: the row's sum, with per-vertex counts a credit word per entry of L (not in the long bin), L, then the matrix
    unsigned long long *rowsum = clique_lds, *credit = clique_lds + 1;
    uint32_t *L = reinterpret_cast<uint32_t *>(credit + (PER && !SLAB ? a.cap : 0u));
    uint32_t *B = SLAB ? a.slab + (size_t)blockIdx.x * a.slab_words : L + a.cap;
    CliqueGroup g;
    g.B = B;
    g.L = L;
    g.credit = SLAB ? a.per : credit;
    g.gl = tid & (uint32_t)(G - 1);
    g.gbase = lane & ~(uint32_t)(G - 1);
    g.mine = 0;
    for (uint32_t it = blockIdx.x; it < a.nitems; it += gridDim.x) {
        const uint32_t v = a.items[it];
        const uint32_t beg = a.row_ptr[v], d = a.row_ptr[v + 1u] - beg;      // d <= cap: the host binned by these very offsets
        if (d < a.min_d) continue;                                           // (the whole workgroup)
        const uint32_t *nv = a.row_idx + (beg - a.nz_base);
        const uint32_t W = (d + 31u) >> 5;
        g.W = W;
        __syncthreads();                                                     // the last row's matrix and credits have been read
        for (uint32_t i = tid; i < d; i += threads) {
            L[i] = nv[i];
            if (PER && !SLAB) credit[i] = 0ull;
        }
        for (uint32_t i = tid; i < d * W; i += threads) B[i] = 0u;
        if (tid == 0u) *rowsum = 0ull;
        if (SLAB) __threadfence();
        __syncthreads();
        // build: a wavefront per row of the matrix
        for (uint32_t i = wave; i < d; i += waves) {
            const uint32_t u = L[i];                                         // < num_rows: established by the plan's first call
            const uint32_t ub = a.row_ptr[u], lu = a.row_ptr[u + 1u] - ub;
            const uint32_t *nu = a.row_idx + (ub - a.nz_base);
            for (uint32_t k = lane; k - lane < lu; k += 64u) {
                if (k < lu) {
                    const uint32_t w = nu[k], at = rows_lower_bound(L, d, w);
                    if (L[at] == w) atomicOr(B + i * W + (at >> 5), 1u << (at & 31u));
                }
            }
        }
        if (SLAB) __threadfence();
        __syncthreads();
        if (a.build_only) continue;
        // count: a group per first-level vertex
        unsigned long long found = 0;
        for (uint32_t i = grp; i < d; i += groups) {
            uint32_t S[WPL];
#pragma unroll
            for (int q = 0; q < WPL; q++) {
                const uint32_t wi = g.gl + (uint32_t)(G * q);
                S[q] = wi < W ? clique_word<SLAB>(B + i * W + wi) : 0u;
            }
            const unsigned long long c = clique_set<K - 3, G, WPL, PER, SLAB>(S, g);
            if (PER) {
                if (g.gl == 0u && c != 0ull) clique_credit<SLAB>(g, i, c);
                found += c;
            }
        }
        if (PER) {
            if (g.gl == 0u && found != 0ull) {
                atomicAdd(rowsum, found);
                g.mine += found;
            }
            __syncthreads();
            // the row's credits: one global add per entry of L that earned any, one for v
            if (!SLAB) {
                for (uint32_t i = tid; i < d; i += threads) {
                    const unsigned long long earned = credit[i];
                    if (earned != 0ull) atomicAdd(a.per + L[i], earned);
                }
            }
            if (tid == 0u && *rowsum != 0ull) atomicAdd(a.per + v, *rowsum);
        }
    }
    clique_total(g.mine, a.total);
}

// ---------------------------------------------------------------------------------------------------------------- the host
// is any v in its own row?  A sequence may then repeat a vertex, and a row shorter than k - 1 is not too short
__global__ __launch_bounds__(256) void clique_diagonal_kernel(const uint32_t *row_ptr, const uint32_t *row_idx, uint32_t nz_base, uint32_t rows,
                                                              uint32_t *found) {
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < rows; v += gridDim.x * blockDim.x) {
        const uint32_t beg = row_ptr[v], d = row_ptr[v + 1u] - beg;
        if (d == 0u) continue;
        const uint32_t *nv = row_idx + (beg - nz_base);
        if (nv[rows_lower_bound(nv, d, v)] == v) atomicOr(found, 1u);
    }
}

template <int K, bool PER>
static int clique_launch_tiny(const CliqueArgs &a, unsigned grid, hipStream_t s) {
    clique_tiny_kernel<K, PER><<<grid, 256, 8u * (PER ? 512u : 256u), s>>>(a);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

template <int K, int G, int WPL, bool PER, bool SLAB>
static int clique_launch(const CliqueArgs &a, unsigned threads, unsigned grid, hipStream_t s) {
    const size_t words = SLAB ? 0u : (size_t)a.cap * ((a.cap + 31u) >> 5);
    const size_t lds = 8u + (PER && !SLAB ? 8u * (size_t)a.cap : 0u) + 4u * (size_t)a.cap + 4u * words;
    if (lds > kCliqueLdsOptIn) {
        static int attr_device = -1;   // per template instantiation; the opt-in is per device (gl_init may switch devices)
        if (attr_device != ctx().device) {
            GL_HIP(hipFuncSetAttribute((const void *)clique_kernel<K, G, WPL, PER, SLAB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kLdsBudget));
            attr_device = ctx().device;
        }
    }
    clique_kernel<K, G, WPL, PER, SLAB><<<grid, threads, lds, s>>>(a);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// the plan's bins, on first use (one synchronisation); a matrix without entries has none: the call only zeroes its outputs
static int clique_prepare(gl_spmv_plan p, const char *who) {
    if (p->nnz == 0 || p->d_clique_scratch) return GL_OK;
    hipStream_t s = ctx().stream;
    const uint32_t rows = p->num_rows;
    // A/B knobs (GRAPHLILY_DEBUG, read by the plan's first call): clique_lds = longest row whose matrix is kept in LDS at all,
    // clique_tiny / clique_mid = longest row of the tiny / mid bin, clique_scratch_mb = room for the long bin's slabs
    const uint32_t cap_lds = (uint32_t)std::max<long>(0, std::min<long>(debug_knob("clique_lds", kCliqueMaxLds), kCliqueMaxLds));
    const uint32_t cap_tiny = (uint32_t)std::max<long>(0, std::min<long>(debug_knob("clique_tiny", kCliqueMaxTiny), std::min(kCliqueMaxTiny, cap_lds)));
    const uint32_t cap_mid = (uint32_t)std::max<long>(0, std::min<long>(debug_knob("clique_mid", kCliqueMaxMid), std::min(kCliqueMaxMid, cap_lds)));
    const uint64_t budget = (uint64_t)std::max<long>(0, std::min<long>(debug_knob("clique_scratch_mb", 1024), 1l << 20)) << 20;
    std::vector<uint32_t> ip((size_t)rows + 1u, 0u);
    // one flag word: does the plan hold a diagonal entry?  Read back behind the synchronisation the offsets need anyway
    uint32_t *flag = nullptr;
    GL_HIP(hipMalloc((void **)&flag, 4));
    hipError_t fe = hipMemsetAsync(flag, 0, 4, s);
    uint32_t diagonal = 0;
    if (fe == hipSuccess) {
        clique_diagonal_kernel<<<rows_stream_grid(rows), 256, 0, s>>>(p->d_csr_indptr, p->d_csr_indices, p->csr_nz_base, rows, flag);
        fe = hipGetLastError();
    }
    if (fe == hipSuccess) fe = hipStreamSynchronize(s);
    if (fe == hipSuccess) fe = hipMemcpy(&diagonal, flag, 4, hipMemcpyDeviceToHost);
    (void)hipFree(flag);
    GL_HIP(fe);
    GL_HIP(hipMemcpy(ip.data(), p->d_csr_indptr, ((size_t)rows + 1u) * 4u, hipMemcpyDeviceToHost));
    const uint32_t shortest = diagonal ? 1u : 2u;      // no k >= 3 finds anything in a shorter row
    auto len = [&](uint32_t v) { return ip[v + 1u] - ip[v]; };
    std::vector<uint32_t> bin[4];
    for (uint32_t v = 0; v < rows; v++) {
        const uint32_t d = len(v);
        if (d < shortest) continue;
        if (d > kCliqueMaxRow)
            return set_error(GL_ERR_UNSUPPORTED,
                             "%s: row %u has %u entries, more than the %u a local bit matrix is built for -- orient the graph by a "
                             "degeneracy rank (io.orient_by_rank with the positions of KCore.run(order=True)): it bounds every row by the degeneracy",
                             who, v, d, kCliqueMaxRow);
        bin[d <= cap_tiny ? 0 : d <= cap_mid ? 1 : d <= cap_lds ? 2 : 3].push_back(v);
    }
    for (auto &b : bin) std::stable_sort(b.begin(), b.end(), [&](uint32_t x, uint32_t y) { return len(x) > len(y); });
    uint32_t cap[4], grid_long = 0, slab_words = 0;
    for (int b = 0; b < 4; b++) cap[b] = bin[b].empty() ? 0u : (len(bin[b][0]) + 1u) & ~1u;
    if (!bin[3].empty()) {
        // a slab per RESIDENT workgroup: the grid is capped so that the slabs stay inside the budget
        slab_words = cap[3] * ((cap[3] + 31u) >> 5);
        const uint64_t fit = budget / (4ull * slab_words);
        if (fit == 0)
            return set_error(GL_ERR_UNSUPPORTED,
                             "%s: the bit matrix of a row of %u entries takes %llu bytes, more than clique_scratch_mb allows (%llu bytes) -- "
                             "orient the graph by a degeneracy rank (io.orient_by_rank with the positions of KCore.run(order=True))",
                             who, cap[3], 4ull * slab_words, (unsigned long long)budget);
        grid_long = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(fit, bin[3].size()), (uint64_t)ctx().num_cus * 2u);
    }
    const size_t words = bin[0].size() + bin[1].size() + bin[2].size() + bin[3].size();
    unsigned char *d_items = nullptr;
    int rc = plan_scratch(d_items, std::max<size_t>(words, 4u) * 4u, who, "row bins");
    if (rc != GL_OK) return rc;
    hipError_t e = hipSuccess;
    size_t at = 0;
    for (auto &b : bin) {
        if (e == hipSuccess && !b.empty())
            e = hipMemcpy(reinterpret_cast<uint32_t *>(d_items) + at, b.data(), b.size() * 4u, hipMemcpyHostToDevice);
        at += b.size();
    }
    if (e == hipSuccess && grid_long) e = hipMalloc((void **)&p->d_clique_slab, (size_t)grid_long * slab_words * 4u);
    if (e != hipSuccess) {
        (void)hipFree(d_items);
        p->d_clique_slab = nullptr;
        return set_error(GL_ERR_HIP, "%s: the row bins and %u slabs of %u words: %s", who, grid_long, slab_words, hipGetErrorString(e));
    }
    p->d_clique_scratch = d_items;
    for (int b = 0; b < 4; b++) {
        p->clique_items[b] = (uint32_t)bin[b].size();
        p->clique_cap[b] = cap[b];
    }
    p->clique_diagonal = diagonal != 0u;
    p->clique_grid_long = grid_long;
    p->clique_slab_words = slab_words;
    return GL_OK;
}

template <int K, bool PER>
static int clique_run(gl_spmv_plan p, CliqueArgs a, uint64_t *launches) {
    hipStream_t s = ctx().stream;
    // A/B knobs (GRAPHLILY_DEBUG, read per call): clique_grid = workgroups per compute unit of the tiny and mid bins,
    // clique_waves = wavefronts of a wide or long workgroup (1 .. 16)
    const unsigned per_cu = (unsigned)std::max<long>(1, std::min<long>(debug_knob("clique_grid", 8), 1024));
    const unsigned wide_threads = 64u * (unsigned)std::max<long>(1, std::min<long>(debug_knob("clique_waves", 16), 16));
    const unsigned most = (unsigned)ctx().num_cus * per_cu;
    const uint32_t *items = reinterpret_cast<const uint32_t *>(p->d_clique_scratch);
    int rc = GL_OK;
    for (int b = 0; b < 4 && rc == GL_OK; b++) {
        a.items = items;
        a.nitems = p->clique_items[b];
        a.cap = p->clique_cap[b];
        items += a.nitems;
        if (a.nitems == 0u || a.cap < a.min_d) continue;                    // (the bin's longest row is too short for this k)
        if (b == 0) rc = clique_launch_tiny<K, PER>(a, std::max(1u, std::min(cdiv(a.nitems, 8u), most)), s);
        else if (b == 1) rc = clique_launch<K, 8, 1, PER, false>(a, 256u, std::min<unsigned>(a.nitems, most), s);
        else if (b == 2) rc = clique_launch<K, 32, 1, PER, false>(a, wide_threads, std::min<unsigned>(a.nitems, (unsigned)ctx().num_cus * 2u), s);
        else rc = clique_launch<K, 64, 4, PER, true>(a, wide_threads, p->clique_grid_long, s);
        ++*launches;
    }
    return rc;
}

template <int K>
static int clique_run_k(gl_spmv_plan p, const CliqueArgs &a, uint64_t *launches) {
    return a.per ? clique_run<K, true>(p, a, launches) : clique_run<K, false>(p, a, launches);
}

static int clique_count(gl_spmv_plan p, uint32_t k, uint64_t *d_total, uint64_t *d_per_vertex, uint64_t *h_stats, const char *who) {
    int rc = rows_require(p, kRowsSets, who, "the plan", "io.orient_by_rank");
    if (rc == GL_OK) rc = clique_prepare(p, who);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    GL_HIP(hipMemsetAsync(d_total, 0, 8, s));
    if (d_per_vertex && p->num_rows) GL_HIP(hipMemsetAsync(d_per_vertex, 0, 8u * (size_t)p->num_rows, s));
    uint64_t launches = 0;
    if (p->d_clique_scratch) {
        CliqueArgs a;
        a.row_ptr = p->d_csr_indptr;
        a.row_idx = p->d_csr_indices;
        a.nz_base = p->csr_nz_base;
        a.total = reinterpret_cast<unsigned long long *>(d_total);
        a.per = reinterpret_cast<unsigned long long *>(d_per_vertex);
        a.slab = p->d_clique_slab;
        a.slab_words = p->clique_slab_words;
        a.items = nullptr;
        a.nitems = a.cap = 0;
        a.min_d = p->clique_diagonal ? 1u : k - 1u;
        a.build_only = debug_knob("clique_build_only", 0) != 0;    // (A/B knob, read per call: what share of a call is the build?)
        switch (k) {
            case 3: rc = clique_run_k<3>(p, a, &launches); break;
            case 4: rc = clique_run_k<4>(p, a, &launches); break;
            case 5: rc = clique_run_k<5>(p, a, &launches); break;
            case 6: rc = clique_run_k<6>(p, a, &launches); break;
            case 7: rc = clique_run_k<7>(p, a, &launches); break;
            default: rc = clique_run_k<8>(p, a, &launches); break;
        }
        if (rc != GL_OK) return rc;
    }
    if (h_stats) {
        h_stats[0] = (uint64_t)p->clique_items[0] + p->clique_items[1];
        h_stats[1] = p->clique_items[2];
        h_stats[2] = p->clique_items[3];
        h_stats[3] = launches;
    }
    return GL_OK;
}

}  // namespace gl

int gl_clique_count(gl_spmv_plan plan, uint32_t k, uint64_t *d_total, uint64_t *d_per_vertex, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_total != nullptr);
    GL_ARG(k >= 3 && k <= 8);
    return gl::clique_count(plan, k, d_total, d_per_vertex, h_stats, "gl_clique_count");
}
