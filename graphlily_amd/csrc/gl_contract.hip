// Graph contraction (gl_contract_symbolic / gl_contract_numeric, graphlily_hip_contract.h): the quotient C = S^T A S of the graph
// in a GL_PLAN_BOOLEAN plan's plain CSR copy by a labelling of its vertices, on square, whole-matrix plans whose rows are strictly
// ascending sets (gl_rows.h: kRowsSets; symmetry is not asked for).  Entry weights travel apart from the plan, a uint32 per entry
// of the row copy; every sum is a 64-bit integer, stored saturated at 0xffffffff and counted.  No floating point anywhere.
//
// RANK   one atomicOr per vertex into a presence bitmap over the labels; a popcount prefix over its words (one workgroup) gives k
//        and part[v] = prefix[label >> 5] + popcount(the bits below label): the groups in ascending order of their labels.
// GROUP  a counting sort of the vertices by part: group sizes and entry bounds by atomics, an exclusive scan into member_ptr,
//        a scatter through per-group cursors.  The order of a group's members depends on the schedule and is invisible: integer
//        adds commute and the rows of C are sorted at emission.
// AGENTS one per group, by a count -- symbolic: the group's entries, an upper bound of |C(a)|; numeric: |C(a)| itself --, the
//        lists compacted in group order by gl_compact.h, as gl_spgemm bins its rows:
//   wavefront   count <= contract_wave_slots (512)    four wavefronts per workgroup, each with its own table; wavefront fences only
//   workgroup   count <= contract_lds_slots (8192)    eight wavefronts share a table in dynamic LDS (96 KiB, hipFuncSetAttribute)
//   slab        above                                 a bitmap and a 64-bit word per column of C in one of a fixed number of global
//                                                     slabs, one per workgroup, cleaned by the group that used it
// THE STREAM.  A group is many short rows, so no lane walks a member: per window of 64 members each lane loads one member's row
// bounds, an inclusive scan of the lengths (shuffles, which the compiler turns into DPP) leaves the 64 exclusive offsets and the
// 64 row starts in LDS, and the lanes take CONSECUTIVE positions of the window's concatenated entries, each finding its member
// by a six-step search in the offsets: index and weight loads are as coalesced as the rows allow and nobody idles behind a hub.
// In the workgroup and slab paths each of the eight wavefronts streams its own windows into the shared table.
// An entry's key is part[column]; the agent's own group is dropped; the slot is claimed by compare-and-swap on 0xffffffff at
// (107 key) mod T with linear probing, the weight added by a 64-bit LDS atomic.  Occupied slots are compacted in place and sorted
// in LDS (counting the smaller keys up to 64 entries, a bitonic network above); the slab emits from its bitmap, in column order.
// tot[a] is a wavefront's sum of k[v] over the members, one writer per word; a k[v] that is not given comes from a pass over
// the rows (a thread per short row, the wavefront for a long one).
// A probe gives up after T slots and emission writes at most the d_c_indptr's room: a d_c_indptr that is not the symbolic call's
// loses entries but writes nothing out of bounds.  Every default is a starting value (EXPERIMENTS.md Round 33).
#include "gl_compact.h"
#include "gl_rows.h"
#include "graphlily_hip_contract.h"

#include <algorithm>

namespace gl {

constexpr uint32_t kContractEmpty = 0xffffffffu;
constexpr uint32_t kContractWaveMax = 512, kContractLdsMax = 8192, kContractMinSlots = 64, kContractRankMax = 64;
constexpr uint32_t kContractWaveThreads = 256, kContractThreads = 512, kContractScanThreads = 1024, kContractScanItems = 4;
constexpr uint32_t kContractWin = 128;               // LDS words of a wavefront's window: 64 offsets, 64 row starts
constexpr uint32_t kContractShortRow = 16;
constexpr uint32_t kContractLdsOptIn = 64u * 1024u;  // what a launch gets without asking
// what an agent computes: the groups' counts from keys alone, C's columns alone, or the summed weights too
enum : int { kContractSymbolic = 0, kContractPattern = 1, kContractWeights = 2 };
// control words (64-bit): k, nnz(C), saturated sums, a label >= num_vertices was seen, a non-empty row behind num_vertices was seen
enum : int { kCtlK = 0, kCtlNnz = 1, kCtlSat = 2, kCtlBadLabel = 3, kCtlBadRow = 4, kCtlWords = 5 };

struct ContractArgs {
    const uint32_t *row_ptr, *row_idx, *part, *weight, *member_ptr, *members;
    const gl_idx_val *items;               // gl_compact.h's list: items[0].index groups, their numbers in items[1 ..].index
    const uint32_t *bound;                 // symbolic: the groups' entries
    const uint32_t *c_ptr;                 // numeric: d_c_indptr
    uint32_t *counts;                      // symbolic: |C(a)| per group (d_c_indptr before the scan)
    uint32_t *c_idx, *c_w;
    unsigned long long *sat;               // the count of saturated sums
    uint32_t *slab_bits;                   // slab path: slab_bits_stride words of bitmap per workgroup ...
    unsigned long long *slab_val;          // ... and slab_val_stride sums; the first slab_words / k of them are used
    uint32_t nz_base, nv, k;
    uint32_t tmax;                         // slots the launch has room for per agent, a power of two
    uint32_t slab_words, slab_bits_stride, slab_val_stride;
};

// ---------------------------------------------------------------------------------------------------------------- the agents
// a wavefront (fences) or a workgroup (barriers) of `size` threads
template <bool WG>
struct ContractTeam {
    uint32_t tid, size;
    __device__ __forceinline__ void sync() const {
        if (WG) {
            __syncthreads();
        } else {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
};
__device__ __forceinline__ void contract_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// exclusive prefix of v over the team, in thread order, the sum in *total; wsum: 17 words of the workgroup's LDS
template <bool WG, typename T>
__device__ __forceinline__ T contract_scan(const ContractTeam<WG> &t, T v, unsigned long long *wsum, T *total) {
    const uint32_t lane = t.tid & 63u;
    T incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const T up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (!WG) {
        *total = __shfl(incl, 63);
        return incl - v;
    }
    const uint32_t w = t.tid >> 6, waves = t.size >> 6;
    if (lane == 63u) wsum[w] = incl;
    __syncthreads();
    T before = 0, sum = 0;
    for (uint32_t i = 0; i < waves; i++) {
        const T c = (T)wsum[i];
        before += i < w ? c : (T)0;
        sum += c;
    }
    __syncthreads();
    *total = sum;
    return before + incl - v;
}

// THE STREAM of group a, run by wavefront `wave` of `waves`: visit(part[column], weight) for every stored entry of every member
// whose column is a labelled vertex.  win: this wavefront's kContractWin words of LDS.  The sum of 64 row lengths is at most nnz,
// which fits 32 bits (rows_require); positions are formed in 64 bits so that none wraps.
template <bool WEIGHTS, typename Visit>
__device__ __forceinline__ void contract_stream(const ContractArgs &g, uint32_t a, uint32_t wave, uint32_t waves, uint32_t lane, uint32_t *win,
                                                Visit &&visit) {
    const uint32_t me = g.member_ptr[a + 1u];
    for (uint64_t base = (uint64_t)g.member_ptr[a] + 64u * wave; base < me; base += 64u * waves) {
        uint32_t beg = 0, len = 0;
        if (base + lane < me) {
            const uint32_t v = g.members[base + lane];                       // < nv <= num_rows: the scatter wrote it
            const uint32_t p0 = g.row_ptr[v];
            beg = p0 - g.nz_base;
            len = g.row_ptr[v + 1u] - p0;
        }
        uint32_t incl = len;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, 63);
        contract_wave_sync();                                                // the last window has been read
        win[lane] = incl - len;
        win[64u + lane] = beg;
        contract_wave_sync();
        for (uint64_t p = lane; p < total; p += 64u) {
            uint32_t j = 0;                                                  // the last member whose offset is <= p: the one that is not empty
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1) j += win[j + step] <= p ? step : 0u;
            const uint32_t e = win[64u + j] + ((uint32_t)p - win[j]);
            const uint32_t col = g.row_idx[e];
            const uint32_t w = WEIGHTS && g.weight ? g.weight[e] : 1u;
            if (col < g.nv) visit(g.part[col], w);                           // (a padding column has no label)
        }
    }
}

__device__ __forceinline__ uint32_t contract_store(const ContractArgs &g, unsigned long long sum) {
    if (sum <= 0xffffffffull) return (uint32_t)sum;
    atomicAdd(g.sat, 1ull);
    return 0xffffffffu;
}

// ------------------------------------------------------------------------------------------------------- the two hash paths
// LDS of a launch, in 64-bit words first: [sums: agents x tmax, with weights only] [17 words of scan room] then 32-bit words:
// [keys: agents x tmax] [one count word, one pad] [the wavefronts' windows: kContractWin each]
template <int MODE, bool WG>
__global__ __launch_bounds__(WG ? kContractThreads : kContractWaveThreads) void contract_hash_kernel(ContractArgs g) {
    extern __shared__ unsigned long long contract_lds[];
    const uint32_t agents = WG ? 1u : blockDim.x >> 6, agent = WG ? 0u : threadIdx.x >> 6;
    ContractTeam<WG> t;
    t.tid = WG ? threadIdx.x : threadIdx.x & 63u;
    t.size = WG ? blockDim.x : 64u;
    unsigned long long *vals = contract_lds + (MODE == kContractWeights ? agent * g.tmax : 0u);
    unsigned long long *wsum = contract_lds + (MODE == kContractWeights ? agents * g.tmax : 0u);
    uint32_t *words = reinterpret_cast<uint32_t *>(wsum + 17);
    uint32_t *keys = words + agent * g.tmax;
    uint32_t *claims = words + agents * g.tmax;
    uint32_t *win = claims + 2 + (threadIdx.x >> 6) * kContractWin;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nitems = g.items[0].index;
    for (uint32_t it = WG ? blockIdx.x : blockIdx.x * agents + agent; it < nitems; it += gridDim.x * agents) {
        const uint32_t a = g.items[1u + it].index;
        const uint32_t out = MODE ? g.c_ptr[a] : 0u;
        const uint32_t count = MODE ? g.c_ptr[a + 1u] - out : g.bound[a];     // 1 .. tmax: the bin's rule
        uint32_t T = kContractMinSlots;
        while (T < g.tmax && T < 2u * count) T <<= 1;
        t.sync();                                                            // the last group's table has been read
        for (uint32_t s = t.tid; s < T; s += t.size) {
            keys[s] = kContractEmpty;
            if (MODE == kContractWeights) vals[s] = 0ull;
        }
        if (WG && t.tid == 0u) *claims = 0u;
        t.sync();
        uint32_t claimed = 0;
        contract_stream<MODE == kContractWeights>(g, a, WG ? threadIdx.x >> 6 : 0u, WG ? blockDim.x >> 6 : 1u, lane, win, [&](uint32_t key, uint32_t w) {
            if (key == a || key >= g.k) return;                              // inside the group: it goes to tot alone (>= k: no symbolic d_part)
            uint32_t h = (key * 107u) & (T - 1u);
            for (uint32_t probe = 0; probe < T; probe++) {
                const uint32_t old = atomicCAS(keys + h, kContractEmpty, key);
                if (old == kContractEmpty || old == key) {
                    if (MODE == kContractWeights) atomicAdd(vals + h, (unsigned long long)w);
                    claimed += old == kContractEmpty ? 1u : 0u;
                    break;
                }
                h = (h + 1u) & (T - 1u);
            }
        });
        if (MODE == kContractSymbolic) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) claimed += __shfl_xor(claimed, off);
            if (WG) {
                if (lane == 0u && claimed) atomicAdd(claims, claimed);
                __syncthreads();
                claimed = *claims;
            }
            if (t.tid == 0u) g.counts[a] = claimed;
            continue;
        }
        t.sync();
        // compact the occupied slots to the front, in place: a piece is read by everyone before anyone writes, and what is
        // written lies in front of the pieces still to be read
        uint32_t have = 0;
        for (uint32_t s0 = 0; s0 < T; s0 += t.size) {
            const uint32_t s = s0 + t.tid;
            const uint32_t key = s < T ? keys[s] : kContractEmpty;
            const unsigned long long val = MODE == kContractWeights && s < T ? vals[s] : 0ull;
            uint32_t total;
            const uint32_t rank = contract_scan<WG, uint32_t>(t, key != kContractEmpty ? 1u : 0u, wsum, &total);
            t.sync();
            if (key != kContractEmpty) {
                keys[have + rank] = key;
                if (MODE == kContractWeights) vals[have + rank] = val;
            }
            have += total;
            t.sync();
        }
        const uint32_t cc = min(have, count);                                // (have == count for the symbolic call's d_c_indptr)
        if (cc <= kContractRankMax) {
            // a short row of C: an entry's place is the number of smaller keys
            if (t.tid < cc) {
                const uint32_t key = keys[t.tid];
                uint32_t r = 0;
                for (uint32_t j = 0; j < cc; j++) r += keys[j] < key ? 1u : 0u;
                g.c_idx[out + r] = key;
                if (MODE == kContractWeights) g.c_w[out + r] = contract_store(g, vals[t.tid]);
            }
            continue;
        }
        uint32_t P = kContractMinSlots;
        while (P < cc) P <<= 1;                                              // <= T: cc <= T and T is a power of two
        for (uint32_t s = cc + t.tid; s < P; s += t.size) keys[s] = kContractEmpty;
        t.sync();
        for (uint32_t k = 2; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t p = t.tid; p < (P >> 1); p += t.size) {
                    const uint32_t lo = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), hi = lo | j;
                    const uint32_t kl = keys[lo], kh = keys[hi];
                    if ((kl > kh) == ((lo & k) == 0u)) {
                        keys[lo] = kh;
                        keys[hi] = kl;
                        if (MODE == kContractWeights) {
                            const unsigned long long v = vals[lo];
                            vals[lo] = vals[hi];
                            vals[hi] = v;
                        }
                    }
                }
                t.sync();
            }
        }
        for (uint32_t s = t.tid; s < cc; s += t.size) {
            g.c_idx[out + s] = keys[s];
            if (MODE == kContractWeights) g.c_w[out + s] = contract_store(g, vals[s]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- the slab path
// a word that atomics of other wavefronts wrote, which the vector cache does not see (gl_clique.hip: clique_word)
template <typename T>
__device__ __forceinline__ T contract_slab_load(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void contract_slab_clear(T *p) {
    __hip_atomic_store(p, (T)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int MODE>
__global__ __launch_bounds__(kContractThreads) void contract_slab_kernel(ContractArgs g) {
    __shared__ unsigned long long wsum[17];
    __shared__ uint32_t wins[(kContractThreads / 64u) * kContractWin];
    ContractTeam<true> t;
    t.tid = threadIdx.x;
    t.size = blockDim.x;
    uint32_t *bits = g.slab_bits + (size_t)blockIdx.x * g.slab_bits_stride;   // all zero between groups
    unsigned long long *vals = g.slab_val + (size_t)blockIdx.x * g.slab_val_stride;
    const uint32_t nitems = g.items[0].index;
    for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        const uint32_t a = g.items[1u + it].index;
        const uint32_t out = MODE ? g.c_ptr[a] : 0u, room = MODE ? g.c_ptr[a + 1u] - out : 0u;
        contract_stream<MODE == kContractWeights>(g, a, threadIdx.x >> 6, blockDim.x >> 6, threadIdx.x & 63u, wins + (threadIdx.x >> 6) * kContractWin,
                                                  [&](uint32_t key, uint32_t w) {                          // key < k: the rank of a label
            if (key == a || key >= g.k) return;
            atomicOr(bits + (key >> 5), 1u << (key & 31u));
            if (MODE == kContractWeights) atomicAdd(vals + key, (unsigned long long)w);
        });
        __threadfence();
        __syncthreads();
        // emit from the bitmap, which is in column order, and leave the slab as it was found
        uint32_t running = 0;
        for (uint32_t w0 = 0; w0 < g.slab_words; w0 += t.size) {
            const uint32_t wi = w0 + t.tid;
            const uint32_t w = wi < g.slab_words ? contract_slab_load(bits + wi) : 0u;
            uint32_t total;
            uint32_t pos = running + contract_scan<true, uint32_t>(t, (uint32_t)__popc(w), wsum, &total);
            if (w != 0u) {
                for (uint32_t r = w; MODE != kContractSymbolic && r; r &= r - 1u, pos++) {
                    const uint32_t c = wi * 32u + (uint32_t)__ffs((int)r) - 1u;
                    unsigned long long acc = 0ull;
                    if (MODE == kContractWeights) {
                        acc = contract_slab_load(vals + c);
                        contract_slab_clear(vals + c);
                    }
                    if (pos < room) {
                        g.c_idx[out + pos] = c;
                        if (MODE == kContractWeights) g.c_w[out + pos] = contract_store(g, acc);
                    }
                }
                contract_slab_clear(bits + wi);
            }
            running += total;
        }
        if (MODE == kContractSymbolic && t.tid == 0u) g.counts[a] = running;
        __threadfence();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------ the streaming passes
__global__ __launch_bounds__(256) void contract_zero_kernel(uint32_t *x, uint64_t words, unsigned long long *ctl, uint32_t ctl_first, uint32_t ctl_words) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) x[i] = 0u;
    if (blockIdx.x == 0u && threadIdx.x < ctl_words) ctl[ctl_first + threadIdx.x] = 0ull;
}

// the labels' presence bits; the two refusals that need a look at the data.  row_ptr == nullptr: a plan without entries
__global__ __launch_bounds__(256) void contract_mark_kernel(const uint32_t *label, const uint32_t *row_ptr, uint32_t nv, uint32_t rows, uint32_t *bits,
                                                            unsigned long long *ctl) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < rows; v += (uint64_t)gridDim.x * blockDim.x) {
        if (v < nv) {
            const uint32_t l = label[v];
            if (l < nv) atomicOr(bits + (l >> 5), 1u << (l & 31u));
            else ctl[kCtlBadLabel] = 1ull;
        } else if (row_ptr && row_ptr[v + 1u] != row_ptr[v]) {
            ctl[kCtlBadRow] = 1ull;
        }
    }
}

// x[0 .. n) -> out[0 .. n] exclusive offsets of f(x) (f: the word, or its popcount; 32 bits each, out may be x), a copy of the
// first n in out2 (may be NULL), the 64-bit sum in *total: one workgroup, four consecutive words per thread and step
template <bool POPCOUNT>
__global__ __launch_bounds__(kContractScanThreads) void contract_scan_kernel(const uint32_t *x, uint32_t n, uint32_t *out, uint32_t *out2, unsigned long long *total) {
    __shared__ unsigned long long wsum[17];
    ContractTeam<true> t;
    t.tid = threadIdx.x;
    t.size = blockDim.x;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += kContractScanThreads * kContractScanItems) {
        const uint64_t i0 = base + (uint64_t)kContractScanItems * t.tid;
        uint32_t f[kContractScanItems];
        unsigned long long mine = 0;
#pragma unroll
        for (uint32_t u = 0; u < kContractScanItems; u++) {
            const uint32_t w = i0 + u < n ? x[i0 + u] : 0u;
            f[u] = POPCOUNT ? (uint32_t)__popc(w) : w;
            mine += f[u];
        }
        unsigned long long sum;
        unsigned long long at = carry + contract_scan<true, unsigned long long>(t, mine, wsum, &sum);
#pragma unroll
        for (uint32_t u = 0; u < kContractScanItems; u++) {
            if (i0 + u < n) {
                out[i0 + u] = (uint32_t)at;
                if (out2) out2[i0 + u] = (uint32_t)at;
            }
            at += f[u];
        }
        carry += sum;
    }
    if (t.tid == 0u) {
        out[n] = (uint32_t)carry;
        *total = carry;
    }
}

// part[v] = the rank of v's label; the group's size and its entries (only run on labels that passed the mark kernel's test)
__global__ __launch_bounds__(256) void contract_part_kernel(const uint32_t *label, const uint32_t *row_ptr, uint32_t nv, const uint32_t *bits,
                                                            const uint32_t *prefix, uint32_t *part, uint32_t *size, uint32_t *bound) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = label[v];
        if (l >= nv) continue;
        const uint32_t a = prefix[l >> 5] + (uint32_t)__popc(bits[l >> 5] & ((1u << (l & 31u)) - 1u));
        part[v] = a;
        atomicAdd(size + a, 1u);
        const uint32_t len = row_ptr ? row_ptr[v + 1u] - row_ptr[v] : 0u;
        if (len) atomicAdd(bound + a, len);
    }
}

__global__ __launch_bounds__(256) void contract_scatter_kernel(const uint32_t *part, uint32_t nv, uint32_t k, uint32_t *cursor, uint32_t *members) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = part[v];
        if (a >= k) continue;                                                // (a d_part that is not the symbolic call's)
        const uint32_t at = atomicAdd(cursor + a, 1u);
        if (at < nv) members[at] = (uint32_t)v;
    }
}

// kv[v] = the summed weights of row v's entries off the diagonal: a thread per short row, the wavefront for a long one
__global__ __launch_bounds__(256) void contract_rowsum_kernel(const uint32_t *row_ptr, const uint32_t *row_idx, uint32_t nz_base, const uint32_t *weight,
                                                              uint32_t nv, unsigned long long *kv) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t v0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; v0 < nv; v0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = v0 + lane;
        uint32_t beg = 0, end = 0;
        if (v < nv) {
            beg = row_ptr[v] - nz_base;
            end = row_ptr[v + 1u] - nz_base;
        }
        unsigned long long sum = 0;
        if (end - beg <= kContractShortRow) {
            for (; beg < end; beg++) {
                const uint32_t col = row_idx[beg];
                if (col < nv && col != v) sum += weight ? weight[beg] : 1u;
            }
        }
        rows_walk_takeover(beg, end, [&](int src, uint32_t b, uint32_t e) {
            const uint32_t vs = (uint32_t)v0 + (uint32_t)src;
            unsigned long long part = 0;
            for (uint64_t j = (uint64_t)b + lane; j < e; j += 64u) {
                const uint32_t col = row_idx[j];
                if (col < nv && col != vs) part += weight ? weight[j] : 1u;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
            if ((int)lane == src) sum = part;
        });
        if (v < nv) kv[v] = sum;
    }
}

// tot[a] = the sum of k[v] over the members of a: a wavefront per group
__global__ __launch_bounds__(256) void contract_tot_kernel(ContractArgs g, const uint32_t *vw, const unsigned long long *kv, uint32_t *tot) {
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t a = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); a < g.k; a += waves) {
        unsigned long long sum = 0;
        for (uint64_t m = (uint64_t)g.member_ptr[a] + lane, me = g.member_ptr[a + 1u]; m < me; m += 64u) {
            const uint32_t v = g.members[m];
            sum += vw ? vw[v] : kv ? kv[v] : 0ull;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0u) tot[a] = contract_store(g, sum);
    }
}

// gl_compact.h's source: the groups whose count -- v[a], or the length of row a of ptr -- lies in (lo, hi]
struct ContractBinSrc {
    const uint32_t *v, *ptr;
    uint32_t n, lo, hi;
    __device__ uint32_t size() const { return n; }
    __device__ bool get(uint32_t i, gl_idx_val &out) const {
        const uint32_t c = ptr ? ptr[i + 1u] - ptr[i] : v[i];
        out.index = i;
        out.val = 0.0f;
        return c > lo && c <= hi;
    }
    __device__ void consumed(uint32_t) const {}
    __device__ void emitted(const gl_idx_val &) const {}
};

// ---------------------------------------------------------------------------------------------------------------- the host
// the plan's scratch, sized by its num_rows n: 256 bytes of control words, n 64-bit vertex weights, then 32-bit arrays
struct ContractScratch {
    unsigned long long *ctl, *kv;
    uint32_t *bits, *prefix, *size, *bound, *member_ptr, *members, *compact;
    gl_idx_val *list[3];               // wavefront, workgroup, slab: symbolic's, then the numeric call's
    size_t zero_words;                 // bits .. bound are one run, cleared by every symbolic call
};
static size_t contract_scratch_map(unsigned char *base, uint32_t n, ContractScratch *m) {
    const size_t bw = cdiv(std::max(n, 1u), 32u);
    size_t at = 256;
    m->ctl = reinterpret_cast<unsigned long long *>(base);
    m->kv = reinterpret_cast<unsigned long long *>(base + at);
    at += (size_t)std::max(n, 1u) * 8u;
    for (auto &l : m->list) {
        l = reinterpret_cast<gl_idx_val *>(base + at);
        at += ((size_t)n + 1u) * 8u;
    }
    auto take = [&](size_t words) {
        uint32_t *p = reinterpret_cast<uint32_t *>(base + at);
        at += words * 4u;
        return p;
    };
    m->bits = take(bw);
    m->size = take(n);
    m->bound = take(n);
    m->zero_words = bw + 2u * (size_t)n;
    m->prefix = take(bw + 1u);
    m->member_ptr = take((size_t)n + 1u);
    m->members = take(std::max(n, 1u));
    m->compact = take((size_t)cdiv(std::max(n, 1u), kCompactChunk) + 2u);
    return at;
}

static uint32_t contract_pow2_floor(long v, uint32_t lo, uint32_t hi) {
    uint32_t p = lo;
    while (p < hi && (long)p * 2 <= v) p <<= 1;
    return p;
}

// three lists over the k groups by the cuts of the plan: counts in (0, wave], (wave, lds], above
static int contract_bin(gl_spmv_plan p, const ContractScratch &m, uint32_t k, const uint32_t *v, const uint32_t *ptr) {
    const uint32_t cut[4] = {0u, p->contract_wave_slots, p->contract_lds_slots, 0xffffffffu};
    for (int b = 0; b < 3; b++) {
        const ContractBinSrc src{v, ptr, k, cut[b], cut[b + 1]};
        const int rc = run_compaction(src, k, m.compact, m.list[b], 0.0f, ctx().stream);
        if (rc != GL_OK) return rc;
    }
    return GL_OK;
}

static int contract_list_sizes(const ContractScratch &m, uint32_t *sizes) {
    for (int b = 0; b < 3; b++) GL_HIP(hipMemcpy(sizes + b, &m.list[b][0].index, 4, hipMemcpyDeviceToHost));
    return GL_OK;
}

template <int MODE, bool WG>
static int contract_launch_hash(const ContractArgs &g, unsigned grid, hipStream_t s) {
    const unsigned threads = WG ? kContractThreads : kContractWaveThreads;
    const size_t agents = WG ? 1u : threads / 64u;
    const size_t lds = (MODE == kContractWeights ? 8u * agents * g.tmax : 0u) + 8u * 17u + 4u * agents * g.tmax + 8u + 4u * (threads / 64u) * kContractWin;
    if (lds > kContractLdsOptIn) {
        static int attr_device = -1;   // per template instantiation; the opt-in is per device (gl_init may switch devices)
        if (attr_device != ctx().device) {
            GL_HIP(hipFuncSetAttribute((const void *)contract_hash_kernel<MODE, WG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
            attr_device = ctx().device;
        }
    }
    contract_hash_kernel<MODE, WG><<<grid, threads, lds, s>>>(g);
    GL_LAUNCH_CHECK();
    return GL_OK;
}

// the three paths over the lists; most[b] = an upper bound of the groups in list b known to the host
template <int MODE>
static int contract_run(gl_spmv_plan p, ContractArgs g, const ContractScratch &m, const uint32_t (&most)[3]) {
    hipStream_t s = ctx().stream;
    // A/B knob (GRAPHLILY_DEBUG, read per call): contract_grid = workgroups per compute unit of the wavefront path (a guess)
    const unsigned per_cu = (unsigned)std::max<long>(1, std::min<long>(debug_knob("contract_grid", 8), 1024));
    const unsigned cus = (unsigned)ctx().num_cus;
    int rc = GL_OK;
    if (most[0] && p->contract_wave_slots) {
        g.items = m.list[0];
        g.tmax = p->contract_wave_slots;
        rc = contract_launch_hash<MODE, false>(g, std::min(cdiv(most[0], kContractWaveThreads / 64u), cus * per_cu), s);
    }
    if (rc == GL_OK && most[1] && p->contract_lds_slots) {
        g.items = m.list[1];
        g.tmax = p->contract_lds_slots;
        rc = contract_launch_hash<MODE, true>(g, std::min(most[1], cus * 2u), s);
    }
    if (rc == GL_OK && most[2] && p->contract_slabs) {
        g.items = m.list[2];
        g.slab_words = cdiv(g.k, 32u);
        g.slab_val_stride = p->num_rows;
        g.slab_bits_stride = cdiv(p->num_rows, 32u);
        g.slab_val = reinterpret_cast<unsigned long long *>(p->d_contract_slab);
        g.slab_bits = reinterpret_cast<uint32_t *>(p->d_contract_slab + 8ull * p->num_rows * p->contract_slabs);
        contract_slab_kernel<MODE><<<std::min(most[2], p->contract_slabs), kContractThreads, 0, s>>>(g);
        GL_LAUNCH_CHECK();
    }
    return rc;
}

static int contract_require(gl_spmv_plan p, uint32_t nv, const char *who) {
    const int rc = rows_require(p, kRowsSets, who, "the plan", "io.symmetrize_simple or io.simple_pattern");
    if (rc != GL_OK) return rc;
    if (nv > p->num_rows) return set_error(GL_ERR_INVALID_ARG, "%s: %u vertices on a plan of %u rows", who, nv, p->num_rows);
    return GL_OK;
}

static ContractArgs contract_args(gl_spmv_plan p, const ContractScratch &m, uint32_t nv, uint32_t k, const uint32_t *d_part) {
    ContractArgs g = {};
    g.row_ptr = p->d_csr_indptr;
    g.row_idx = p->d_csr_indices;
    g.nz_base = p->csr_nz_base;
    g.part = d_part;
    g.member_ptr = m.member_ptr;
    g.members = m.members;
    g.bound = m.bound;
    g.sat = m.ctl + kCtlSat;
    g.nv = nv;
    g.k = k;
    return g;
}

// slabs for the groups no table holds: one per RESIDENT workgroup, all zero between groups, sized by the plan's rows (k is at
// most that), so that every later call finds the same grid
static int contract_slabs(gl_spmv_plan p, const char *who) {
    if (p->d_contract_slab) return GL_OK;
    const uint32_t n = p->num_rows;
    // A/B knob (GRAPHLILY_DEBUG): contract_scratch_mb = room for the slabs (a guess)
    const uint64_t budget = (uint64_t)std::max<long>(0, std::min<long>(debug_knob("contract_scratch_mb", 1024), 1l << 20)) << 20;
    const uint64_t per_slab = 4ull * cdiv(n, 32u) + 8ull * n;
    const uint64_t slabs = std::min<uint64_t>(budget / per_slab, (uint64_t)ctx().num_cus);
    if (slabs == 0)
        return set_error(GL_ERR_UNSUPPORTED, "%s: a dense accumulator over %u columns takes %llu bytes, more than contract_scratch_mb allows (%llu bytes)",
                         who, n, (unsigned long long)per_slab, (unsigned long long)budget);
    const hipError_t e = hipMalloc((void **)&p->d_contract_slab, slabs * per_slab);
    if (e != hipSuccess) return set_error(GL_ERR_HIP, "%s: %llu slabs of %llu bytes: %s", who, (unsigned long long)slabs, (unsigned long long)per_slab, hipGetErrorString(e));
    GL_HIP(hipMemsetAsync(p->d_contract_slab, 0, slabs * per_slab, ctx().stream));
    p->contract_slabs = (uint32_t)slabs;
    return GL_OK;
}

static int contract_symbolic(gl_spmv_plan p, uint32_t nv, const uint32_t *d_label, uint32_t *d_part, uint32_t *d_c_indptr, uint64_t *h_stats,
                             const char *who) {
    int rc = contract_require(p, nv, who);
    if (rc != GL_OK) return rc;
    hipStream_t s = ctx().stream;
    const uint32_t n = p->num_rows;
    for (int i = 0; i < 6; i++) h_stats[i] = 0;
    p->contract_k = 0xffffffffu;                                             // no numeric call until this one has succeeded
    ContractScratch m;
    const size_t bytes = contract_scratch_map(nullptr, n, &m);
    const bool fresh = p->d_contract_scratch == nullptr;
    if ((rc = plan_scratch(p->d_contract_scratch, bytes, who, "groups and bin lists")) != GL_OK) return rc;
    contract_scratch_map(p->d_contract_scratch, n, &m);
    if (fresh) GL_HIP(hipMemsetAsync(m.compact, 0, 4, s));                    // gl_compact.h's ticket
    // A/B knobs (GRAPHLILY_DEBUG, read by every symbolic call and kept for the numeric call behind it): contract_wave /
    // contract_lds = 0 close the wavefront path / both hash paths, contract_wave_slots / contract_lds_slots = their tables
    // (powers of two from 64).  ALL GUESSES.
    const bool use_lds = debug_knob("contract_lds", 1) != 0, use_wave = use_lds && debug_knob("contract_wave", 1) != 0;
    const uint32_t lds_slots = contract_pow2_floor(debug_knob("contract_lds_slots", kContractLdsMax), kContractMinSlots, kContractLdsMax);
    const uint32_t wave_slots = std::min(lds_slots, contract_pow2_floor(debug_knob("contract_wave_slots", kContractWaveMax), kContractMinSlots, kContractWaveMax));
    p->contract_lds_slots = use_lds ? lds_slots : 0u;
    p->contract_wave_slots = use_wave ? wave_slots : 0u;
    const uint32_t *row_ptr = p->nnz ? p->d_csr_indptr : nullptr;
    const uint32_t bw = cdiv(std::max(n, 1u), 32u);
    contract_zero_kernel<<<rows_stream_grid((uint32_t)std::min<size_t>(m.zero_words, 0xffffffffu)), 256, 0, s>>>(m.bits, m.zero_words, m.ctl, 0u, kCtlWords);
    GL_LAUNCH_CHECK();
    contract_mark_kernel<<<rows_stream_grid(n), 256, 0, s>>>(d_label, row_ptr, nv, n, m.bits, m.ctl);
    GL_LAUNCH_CHECK();
    contract_scan_kernel<true><<<1, kContractScanThreads, 0, s>>>(m.bits, bw, m.prefix, nullptr, m.ctl + kCtlK);
    GL_LAUNCH_CHECK();
    GL_HIP(hipStreamSynchronize(s));
    unsigned long long ctl[kCtlWords];
    GL_HIP(hipMemcpy(ctl, m.ctl, sizeof(ctl), hipMemcpyDeviceToHost));
    if (ctl[kCtlBadLabel]) return set_error(GL_ERR_INVALID_ARG, "%s: a label is at or above num_vertices (%u): labels are vertex numbers", who, nv);
    if (ctl[kCtlBadRow])
        return set_error(GL_ERR_UNSUPPORTED, "%s: a row at or behind num_vertices (%u) is not empty: only padding vertices may follow the labelled ones", who, nv);
    const uint32_t k = (uint32_t)ctl[kCtlK];
    contract_part_kernel<<<rows_stream_grid(nv), 256, 0, s>>>(d_label, row_ptr, nv, m.bits, m.prefix, d_part, m.size, m.bound);
    GL_LAUNCH_CHECK();
    contract_scan_kernel<false><<<1, kContractScanThreads, 0, s>>>(m.size, k, m.member_ptr, m.size, m.ctl + kCtlNnz);
    GL_LAUNCH_CHECK();
    contract_scatter_kernel<<<rows_stream_grid(nv), 256, 0, s>>>(d_part, nv, k, m.size, m.members);
    GL_LAUNCH_CHECK();
    contract_zero_kernel<<<rows_stream_grid(k + 1u), 256, 0, s>>>(d_c_indptr, (uint64_t)k + 1u, m.ctl, kCtlNnz, 1u);
    GL_LAUNCH_CHECK();
    uint32_t bins[3] = {0, 0, 0};
    unsigned long long nnz = 0;
    if (p->nnz) {
        if ((rc = contract_bin(p, m, k, m.bound, nullptr)) != GL_OK) return rc;
        GL_HIP(hipStreamSynchronize(s));
        if ((rc = contract_list_sizes(m, bins)) != GL_OK) return rc;
        if (bins[2] && (rc = contract_slabs(p, who)) != GL_OK) return rc;
        ContractArgs g = contract_args(p, m, nv, k, d_part);
        g.counts = d_c_indptr;
        if ((rc = contract_run<kContractSymbolic>(p, g, m, bins)) != GL_OK) return rc;
        contract_scan_kernel<false><<<1, kContractScanThreads, 0, s>>>(d_c_indptr, k, d_c_indptr, nullptr, m.ctl + kCtlNnz);
        GL_LAUNCH_CHECK();
        GL_HIP(hipStreamSynchronize(s));
        GL_HIP(hipMemcpy(&nnz, m.ctl + kCtlNnz, 8, hipMemcpyDeviceToHost));
    } else {
        GL_HIP(hipStreamSynchronize(s));
    }
    h_stats[0] = k;
    h_stats[1] = nnz;
    h_stats[2] = p->nnz;
    h_stats[3] = bins[1];
    h_stats[4] = bins[2];
    if (nnz > 0xffffffffull) return set_error(GL_ERR_UNSUPPORTED, "%s: C has %llu entries, which do not fit 32-bit offsets", who, nnz);
    p->contract_k = k;
    p->contract_nv = nv;
    for (int b = 0; b < 3; b++) p->contract_bins[b] = bins[b];
    return GL_OK;
}

static int contract_numeric(gl_spmv_plan p, uint32_t nv, const uint32_t *d_part, uint32_t k, const uint32_t *d_weight, const uint32_t *d_vertex_weight,
                            const uint32_t *d_c_indptr, uint32_t *d_c_indices, uint32_t *d_c_weight, uint32_t *d_tot, uint64_t *h_stats, const char *who) {
    int rc = contract_require(p, nv, who);
    if (rc != GL_OK) return rc;
    if (h_stats)
        for (int i = 0; i < 6; i++) h_stats[i] = 0;
    if (!p->d_contract_scratch || p->contract_k != k || p->contract_nv != nv)
        return set_error(GL_ERR_INVALID_ARG, "%s: k = %u over %u vertices is not what the plan's last gl_contract_symbolic call found: the grouping it "
                         "left in the plan is the one this call walks", who, k, nv);
    hipStream_t s = ctx().stream;
    ContractScratch m;
    contract_scratch_map(p->d_contract_scratch, p->num_rows, &m);
    ContractArgs g = contract_args(p, m, nv, k, d_part);
    g.weight = d_weight;
    g.c_ptr = d_c_indptr;
    g.c_idx = d_c_indices;
    g.c_w = d_c_weight;
    contract_zero_kernel<<<1, 256, 0, s>>>(nullptr, 0u, m.ctl, kCtlSat, 1u);
    GL_LAUNCH_CHECK();
    if (p->nnz && k) {
        if ((rc = contract_bin(p, m, k, nullptr, d_c_indptr)) != GL_OK) return rc;
        // |C(a)| <= the group's entries, so a list by |C(a)| holds no more groups than the symbolic lists from its own path upwards
        const uint32_t *sb = p->contract_bins;
        const uint32_t most[3] = {sb[0] + sb[1] + sb[2], sb[1] + sb[2], sb[2]};
        rc = d_c_weight ? contract_run<kContractWeights>(p, g, m, most) : contract_run<kContractPattern>(p, g, m, most);
        if (rc != GL_OK) return rc;
    }
    if (d_tot && k) {
        const bool derive = !d_vertex_weight && p->nnz;
        if (derive) {
            contract_rowsum_kernel<<<rows_stream_grid(nv), 256, 0, s>>>(p->d_csr_indptr, p->d_csr_indices, p->csr_nz_base, d_weight, nv, m.kv);
            GL_LAUNCH_CHECK();
        }
        contract_tot_kernel<<<rows_stream_grid(std::min<uint64_t>(64ull * k, 0xffffffffull)), 256, 0, s>>>(g, d_vertex_weight, derive ? m.kv : nullptr, d_tot);
        GL_LAUNCH_CHECK();
    }
    if (!h_stats) return GL_OK;
    GL_HIP(hipStreamSynchronize(s));
    uint32_t sizes[3] = {0, 0, 0}, nnz = 0;
    unsigned long long sat = 0;
    if (p->nnz && k && (rc = contract_list_sizes(m, sizes)) != GL_OK) return rc;
    GL_HIP(hipMemcpy(&nnz, d_c_indptr + k, 4, hipMemcpyDeviceToHost));
    GL_HIP(hipMemcpy(&sat, m.ctl + kCtlSat, 8, hipMemcpyDeviceToHost));
    h_stats[0] = k;
    h_stats[1] = nnz;
    h_stats[2] = p->nnz;
    h_stats[3] = sizes[1];
    h_stats[4] = sizes[2];
    h_stats[5] = sat;
    return GL_OK;
}

}  // namespace gl

int gl_contract_symbolic(gl_spmv_plan plan, uint32_t num_vertices, const uint32_t *d_label, uint32_t *d_part, uint32_t *d_c_indptr, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_label != nullptr && d_part != nullptr && d_c_indptr != nullptr && h_stats != nullptr);
    return gl::contract_symbolic(plan, num_vertices, d_label, d_part, d_c_indptr, h_stats, "gl_contract_symbolic");
}

int gl_contract_numeric(gl_spmv_plan plan, uint32_t num_vertices, const uint32_t *d_part, uint32_t k, const uint32_t *d_weight, const uint32_t *d_vertex_weight,
                        const uint32_t *d_c_indptr, uint32_t *d_c_indices, uint32_t *d_c_weight, uint32_t *d_tot, uint64_t *h_stats) {
    GL_TRACE();
    GL_REQUIRE_INIT();
    GL_ARG(plan != nullptr && d_part != nullptr && d_c_indptr != nullptr && d_c_indices != nullptr);
    return gl::contract_numeric(plan, num_vertices, d_part, k, d_weight, d_vertex_weight, d_c_indptr, d_c_indices, d_c_weight, d_tot, h_stats,
                                "gl_contract_numeric");
}
